"""f-14 without a GPU: the host twins of the dense information matrix and of the robust pose-graph optimiser
(csrc/posegraph_cpu.cpp) against the numpy restatement of tests/posegraph_oracle.py, and the Python surface around them
(usip_amd/posegraph.py, fragments.register_pairs_cpu / summarize).

Tolerances.  The twin and the oracle compute the same mathematics with different roundings, so they are compared within 1000
times the oracle's OWN noise (f-13's factor), and that noise is measured, not chosen: for the optimiser the largest
difference between two oracle runs that enter the unknowns into the linear system in ascending and in descending fragment
order; for the information the rows added forward against reversed.  A measured noise of exactly zero (the two-fragment scene
has one block) is raised to one unit in the last place of the largest compared value, below which no float64 result can
differ.  The energy f reaches 1e4 for a false loop closure, so it is compared relative to max(1, |f|).  Every bound must
itself stay below 1e-9."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import posegraph_oracle as po
from usip_amd import fragments as fr, posegraph as pg

FACTOR, CEILING = 1000.0, 1e-9


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def oracle():
    """name -> (scene, ascending run, descending run), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            sc = po.SCENES[name]()
            it1, it2 = po.ITERATIONS[name]
            run = lambda d: po.optimise(sc["n"], sc["edges"], sc["X"], sc["L"], sc["T0"], iterations1=it1, iterations2=it2,
                                        descending=d)
            cache[name] = (sc, run(False), run(True))
        return cache[name]
    return get


def twin(scenes, it, threads=1, **kw):
    return pg.optimize_arrays_cpu(po.batch_of(scenes), iterations1=it[0], iterations2=it[1], num_threads=threads, **kw)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@pytest.mark.parametrize("name", sorted(po.SCENES))
def test_fixture_is_decisive_and_the_twin_matches_the_oracle(oracle, name):
    sc, o, o2 = oracle(name)
    E, n = len(sc["edges"]), sc["n"]
    loops = np.array([j - i > 1 for i, j in sc["edges"]], bool)
    # the oracle's own result: no decision near the threshold, and the planted truth comes out
    assert not np.any(np.abs(o["weight1"][loops] - 0.25) < 0.05), o["weight1"][loops]
    assert np.array_equal(o["kept"], sc["truth"])
    r = twin([sc], po.ITERATIONS[name])
    assert r["status"][0] == o["status"] == 0
    assert np.array_equal(r["kept"][0, :E], o["kept"]) and np.array_equal(r["iterations_done"][0], o["iterations_done"])
    for key, got, a, b, relative in (("T", r["T"][0, :n], o["T"], o2["T"], False),
                                     ("weight1", r["weight1"][0, :E], o["weight1"], o2["weight1"], False),
                                     ("weight2", r["weight2"][0, :E], o["weight2"], o2["weight2"], False),
                                     ("energy", r["energy"][0, :E], o["energy"], o2["energy"], True)):
        if E == 0 and key != "T":
            continue
        diff = rel if relative else (lambda x, y: np.abs(x - y))
        scale = 1.0 if relative else max(1.0, float(np.abs(a).max()))
        noise = max(float(diff(b, a).max()), np.spacing(scale))
        bound = FACTOR * noise
        err = float(diff(got, a).max())
        print("%s %s: oracle noise %.2e, bound %.2e, twin - oracle %.2e" % (name, key, noise, bound, err))
        assert bound < CEILING and err <= bound, key
    assert np.all(np.isfinite(r["last_step"])) and abs(r["last_step"][0, 0] - o["last_step"][0]) <= 1e-9
    # zeros beyond n and ecount never arise here (one scene, exact shapes); the ragged batch below checks them


def test_quaternion_branches_are_all_taken():
    """The exact-entry turns reach the three branches the trace does not, and the sign flip."""
    seen, flipped = set(), False
    for name in ("half_x", "half_y", "half_z", "third_111", "4/2/1"):
        sc = po.SCENES[name]()
        T = [po.to4(t) for t in sc["T0"]]
        for k, (i, j) in enumerate(sc["edges"]):
            D = po.rigid_inv(T[i]) @ T[j] @ po.rigid_inv(po.to4(sc["X"][k]))
            _, b, flip = po.quat_vector(D[:3, :3])
            seen.add(b)
            flipped = flipped or bool(flip)
    assert seen == {0, 1, 2, 3} and flipped


def test_threads_and_a_ragged_batch_change_nothing(oracle):
    names = ["12/14/8", "2/0/0", "4/2/1"]
    scenes = [oracle(n)[0] for n in names]
    one, many = twin(scenes, (8, 3), 1), twin(scenes, (8, 3), 16)
    for k in one:
        assert np.array_equal(bits(one[k]), bits(many[k])), k
    for s, sc in enumerate(scenes):
        alone = twin([sc], (8, 3))
        E, n = len(sc["edges"]), sc["n"]
        for k in ("weight1", "weight2", "energy", "kept"):
            assert np.array_equal(bits(one[k][s, :E]), bits(alone[k][0])), k
            assert not one[k][s, E:].any(), k                          # zeros beyond ecount
        assert np.array_equal(bits(one["T"][s, :n]), bits(alone["T"][0])) and not one["T"][s, n:].any()
        for k in ("iterations_done", "last_step", "status"):
            assert np.array_equal(bits(one[k][s]), bits(alone[k][0])), k


def graph_lists(sc):
    odom, odom_info, loop, loop_info = [], [], [], []
    for k, (i, j) in enumerate(sc["edges"]):
        tag = (i, j, sc["n"])
        (odom if j - i == 1 else loop).append(fr.LogEntry(tag, po.to4(sc["X"][k])))
        (odom_info if j - i == 1 else loop_info).append(fr.InfoEntry(tag, sc["L"][k]))
    return odom, odom_info, loop, loop_info


def test_edges_given_to_python_in_any_order_give_the_same_result(oracle):
    sc = oracle("12/14/8")[0]
    lists = graph_lists(sc)
    g = pg.build_graph(*lists)
    assert g.n == sc["n"] and list(zip(g.edge_i.tolist(), g.edge_j.tolist())) == sc["edges"]
    assert np.array_equal(bits(g.X), bits(sc["X"])) and np.allclose(g.T0, sc["T0"], rtol=0, atol=1e-13)
    rng = np.random.default_rng(0)
    shuffled = []
    for a, b in ((lists[0], lists[1]), (lists[2], lists[3])):
        order = rng.permutation(len(a))
        shuffled += [[a[k] for k in order], [b[k] for k in order]]
    r1, = pg.optimize_cpu([g], iterations1=8, iterations2=3)
    r2, = pg.optimize_cpu([pg.build_graph(*shuffled)], iterations1=8, iterations2=3)
    for a, b in zip(r1, r2):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    both = twin([sc], (8, 3))
    assert np.array_equal(r1.kept, both["kept"][0]) and r1.status == 0
    # what build_graph refuses
    for bad, what in ((lambda: pg.build_graph(lists[0][1:], lists[1][1:], lists[2], lists[3]), "lacks the pair \\(0, 1\\)"),
                      (lambda: pg.build_graph(lists[0] + lists[0][:1], lists[1] + lists[1][:1], lists[2], lists[3]), "twice"),
                      (lambda: pg.build_graph([fr.LogEntry((1, 0, 2), np.eye(4))], [fr.InfoEntry((1, 0, 2), np.eye(6))], [], []),
                       "i < j")):
        with pytest.raises(ValueError, match=what):
            bad()


def test_every_limit_is_refused(oracle):
    sc = oracle("4/2/1")[0]
    b = po.batch_of([sc])
    ok = lambda **kw: pg.optimize_arrays_cpu(dict(b, **kw.pop("arrays", {})), **kw)
    assert ok(iterations1=0, iterations2=0)["status"][0] == 0 and ok(iterations1=256, iterations2=0)["status"][0] == 0
    for kw in (dict(tau2=0.0), dict(tau2=-1.0), dict(tau2=float("nan")), dict(tau2=float("inf")), dict(prune=-0.1),
               dict(prune=1.5), dict(iterations1=-1), dict(iterations1=257), dict(iterations2=-1), dict(iterations2=257)):
        with pytest.raises(RuntimeError, match="USIP_EINVAL"):
            ok(**kw)
    E = len(sc["edges"])
    swapped_i, swapped_j = b["edge_i"].copy(), b["edge_j"].copy()
    swapped_i[0, [0, 1]], swapped_j[0, [0, 1]] = swapped_i[0, [1, 0]], swapped_j[0, [1, 0]]
    twice_i, twice_j = b["edge_i"].copy(), b["edge_j"].copy()
    twice_i[0, 1], twice_j[0, 1] = twice_i[0, 0], twice_j[0, 0]
    bad = [dict(n=np.array([1], np.int32)), dict(n=np.array([5], np.int32)), dict(ecount=np.array([E + 1], np.int32)),
           dict(ecount=np.array([-1], np.int32)), dict(edge_i=swapped_i, edge_j=swapped_j), dict(edge_i=twice_i, edge_j=twice_j),
           dict(edge_i=b["edge_j"], edge_j=b["edge_i"]), dict(edge_j=np.where(b["edge_j"] == 3, 4, b["edge_j"]).astype(np.int32))]
    for arrays in bad:
        with pytest.raises(RuntimeError, match="USIP_EINVAL"):
            ok(arrays=arrays)
    big = po.batch_of([sc])
    wide = {k: np.zeros((1, 7) + v.shape[2:], v.dtype) for k, v in big.items() if k in ("edge_i", "edge_j", "X", "info")}
    with pytest.raises(RuntimeError, match="USIP_EINVAL"):            # Emax above Nmax (Nmax - 1) / 2
        pg.optimize_arrays_cpu(dict(big, **wide))
    with pytest.raises(RuntimeError, match="USIP_EINVAL"):            # Nmax above 128
        pg.optimize_arrays_cpu(dict(big, T0=np.zeros((1, 129, 3, 4))))
    with pytest.raises(RuntimeError):
        pg.optimize_cpu([pg.build_graph(*graph_lists(sc))], tau2=0.0)


def test_a_missing_odometry_edge_ends_with_a_status_and_finite_poses(oracle):
    """At the C level nothing asks for a connected graph: fragment 3 without any edge has a zero diagonal block."""
    sc = dict(oracle("4/2/1")[0])
    keep = [k for k, (i, j) in enumerate(sc["edges"]) if 3 not in (i, j)]
    sc.update(edges=[sc["edges"][k] for k in keep], X=sc["X"][keep], L=sc["L"][keep])
    r = twin([sc], (6, 2))
    assert r["status"][0] == 1 and r["iterations_done"][0].tolist() == [0, 0]
    assert np.array_equal(bits(r["T"][0]), bits(sc["T0"])) and np.all(np.isfinite(r["weight1"])) and np.all(np.isfinite(r["energy"]))
    # a transform that is no rotation at all: still no NaN leaves the call
    sc2 = dict(oracle("4/2/1")[0])
    X = sc2["X"].copy()
    X[1] = 0.0
    sc2["X"] = X
    r = twin([sc2], (6, 2))
    for k in ("T", "weight1", "weight2", "energy", "last_step"):
        assert np.all(np.isfinite(r[k])), k
    assert r["status"][0] in (0, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ the information matrix
@pytest.fixture(scope="module")
def info_case():
    clouds, pairs = po.information_bank()
    bank = fr.host_bank(clouds)
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    rng = np.random.default_rng(2)
    Rt = np.tile(np.eye(3, 4), (len(pairs), 1, 1))
    Rt[:7, :, 3] = rng.normal(size=(7, 3)) * 0.02
    Rt[13, :, 3] = 10.0                                                # nothing within the radius
    mask = np.ones(len(pairs), np.uint8)
    mask[10] = 0
    idx, d2 = fr.icp_nearest_cpu(bank, f1, f2, Rt, mask)
    return clouds, pairs, bank, f1, f2, mask, idx, d2


def test_information_twin_matches_the_oracle(info_case):
    clouds, pairs, bank, f1, f2, mask, idx, d2 = info_case
    F = len(clouds)
    for radius in (0.12, po.LATTICE_RADIUS):
        info, count = pg.icp_information_cpu(bank, f1, f2, idx, d2, mask, radius)
        info16, count16 = pg.icp_information_cpu(bank, f1, f2, idx, d2, mask, radius, num_threads=16)
        assert np.array_equal(bits(info), bits(info16)) and np.array_equal(count, count16)
        assert np.array_equal(bits(info), bits(np.swapaxes(info, 1, 2))) and np.all(np.isfinite(info))     # exactly symmetric
        for p, (a, b) in enumerate(pairs):
            a, b = min(max(a, 0), F - 1), min(max(b, 0), F - 1)        # ids outside the bank behave as the nearer end
            n1, n2 = len(clouds[a]), len(clouds[b])
            if mask[p] == 0 or n1 == 0 or n2 == 0:
                assert count[p] == 0 and not info[p].any(), p
                continue
            want, n = po.information(clouds[a], idx[p, :n2], d2[p, :n2], radius)
            back, _ = po.information(clouds[a], idx[p, :n2], d2[p, :n2], radius, reverse=True)
            assert count[p] == n and info[p, 0, 0] == n, p
            noise = max(float(np.abs(want - back).max()), np.spacing(max(1.0, float(np.abs(want).max()))))
            bound = FACTOR * noise
            err = float(np.abs(info[p] - want).max())
            print("pair %d (%d rows, %d within %.4f): oracle noise %.2e, bound %.2e, twin - oracle %.2e" % (p, n2, n, radius,
                                                                                                       noise, bound, err))
            assert bound < CEILING and err <= bound, p
    assert count[13] == 0 and not info[13].any()                       # nothing within the radius: zeros, never a NaN
    assert count[po.LATTICE_PAIR] == po.LATTICE_COUNT                   # 2/64 counts, exactly 3/64 and 4/64 do not
    assert count[9] == len(clouds[7])                                  # the lattice on itself: every distance is 0
    several = np.bincount(idx[5, :len(clouds[6])])                     # every query on the one row of fragment 1
    assert several.tolist() == [len(clouds[6])]
    with pytest.raises(RuntimeError):
        pg.icp_information_cpu(bank, f1, f2, idx, d2, mask, 0.0)
    with pytest.raises(RuntimeError):
        pg.icp_information_cpu(bank, np.zeros(65536, np.int32), np.zeros(65536, np.int32), np.zeros((65536, 1), np.int32),
                               np.zeros((65536, 1)))


# ------------------------------------------------------------------------------------------------ the Python surface
def test_split_entries_follows_the_script_line_by_line():
    """Five fragments; the log holds (0,1), (2,3), (0,2), (1,4) in that order; gt.log holds every pair of the chain and (0,2)."""
    n = 5
    T = lambda v: np.vstack((np.hstack((np.eye(3), [[v], [0.0], [0.0]])), [0, 0, 0, 1.0]))
    log = [fr.ResultEntry((i, j, n), T(10 * i + j), 7, 0.5, np.eye(6)) for i, j in ((0, 1), (2, 3), (0, 2), (1, 4))]
    infos = [fr.InfoEntry(e.info, np.eye(6) * (k + 1)) for k, e in enumerate(log)]
    gt = [fr.LogEntry((i, j, n), T(100 + 10 * i + j)) for i, j in ((0, 1), (0, 2), (1, 2), (2, 3), (3, 4))]
    gt_info = [fr.InfoEntry(g.info, np.eye(6) * (50 + k)) for k, g in enumerate(gt)]
    odom, odom_info, loop, loop_info = pg.split_entries(log, infos, n, gt, gt_info, "gt")
    # the script: the log's own order, then gt's order for what the odometry list lacks
    assert [e.info for e in odom] == [(0, 1, n), (2, 3, n), (1, 2, n), (3, 4, n)] == [e.info for e in odom_info]
    assert [e.info for e in loop] == [(0, 2, n), (1, 4, n)] == [e.info for e in loop_info]
    assert odom[0].trans[0, 3] == 1 and odom[1].trans[0, 3] == 23 and odom[2].trans[0, 3] == 112 and odom[3].trans[0, 3] == 134
    assert [m.mat[0, 0] for m in odom_info] == [1, 2, 52, 54]          # a filled edge carries gt.info's matrix
    assert [m.mat[0, 0] for m in loop_info] == [3, 4] and loop[1].trans[0, 3] == 14
    est = {(1, 2): (T(-1), np.eye(6) * 9), (3, 4): (T(-2), np.eye(6) * 8), (0, 1): (T(-3), np.eye(6))}
    odom, odom_info, _, _ = pg.split_entries(log, infos, n, fill="estimate", estimates=est)
    assert [e.info[:2] for e in odom] == [(0, 1), (2, 3), (1, 2), (3, 4)] and odom[0].trans[0, 3] == 1
    assert [m.mat[0, 0] for m in odom_info] == [1, 2, 9, 8] and odom[2].trans[0, 3] == -1
    with pytest.raises(ValueError, match="lacks the pair \\(1, 2\\)"):
        pg.split_entries(log, infos, n, fill=None)
    with pytest.raises(ValueError, match="lacks the pair \\(3, 4\\)"):
        pg.split_entries(log, infos, n, fill="estimate", estimates={(1, 2): est[(1, 2)]})
    with pytest.raises(ValueError):
        pg.split_entries(log, infos[:-1], n, gt, gt_info)


def test_files_are_written_read_back_and_equal(tmp_path, oracle):
    sc = oracle("12/14/8")[0]
    lists = graph_lists(sc)
    paths = pg.write_split(tmp_path, "room", *lists)
    assert [os.path.basename(p) for p in paths] == ["room_odom.log", "room_odom.info", "room_loop.log", "room_loop.info"]
    back = pg.read_split(tmp_path, "room")
    for want, got in zip(lists, back):
        assert [tuple(e.info) for e in want] == [tuple(e.info) for e in got]
        for a, b in zip(want, got):
            assert np.allclose(a[1], b[1], rtol=1e-8, atol=1e-8)       # %.8e and %.8f, the reference's formats
    again = pg.write_split(tmp_path, "again", *back)
    for p, q in zip(paths, again):
        assert open(p).read() == open(q).read()                       # what was read is written back byte for byte
    g = pg.build_graph(*lists)
    r, = pg.optimize_cpu([g], iterations1=8, iterations2=3)
    entries = pg.refined_entries(g, r)
    path = pg.write_refined(tmp_path, "room", entries)
    assert os.path.basename(path) == "room_reg_refine_all.log"
    got = fr.read_log(path)
    assert [tuple(e.info) for e in got] == [tuple(e.info) for e in entries]


def test_refined_entries_hold_the_kept_edges_under_either_transform(oracle):
    sc = oracle("12/14/8")[0]
    g = pg.build_graph(*graph_lists(sc))
    r, = pg.optimize_cpu([g], iterations1=10, iterations2=3)
    want = [k for k, (i, j) in enumerate(sc["edges"]) if j - i == 1 or sc["truth"][k]]
    edge, graph = pg.refined_entries(g, r, "edge"), pg.refined_entries(g, r, "graph")
    assert [e.info for e in edge] == [(sc["edges"][k] + (sc["n"],)) for k in want] == [e.info for e in graph]
    for e, q, k in zip(edge, graph, want):
        i, j = sc["edges"][k]
        assert np.array_equal(e.trans[:3], sc["X"][k]) and np.array_equal(e.trans[3], [0, 0, 0, 1])
        rel_pose = po.rigid_inv(po.to4(r.T[i])) @ po.to4(r.T[j])
        assert np.allclose(q.trans, rel_pose, rtol=0, atol=1e-12) and np.allclose(q.trans, e.trans, rtol=0, atol=0.05)
    with pytest.raises(ValueError):
        pg.refined_entries(g, r, "pose")
    # scored as mrEvaluateRegistration scores: the truth as ground truth, every kept loop closure is good
    gt = [fr.LogEntry((i, j, sc["n"]), po.to4(sc["X"][k])) for k, (i, j) in enumerate(sc["edges"]) if sc["truth"][k]]
    gt_info = [fr.InfoEntry(e.info, sc["L"][k]) for e, k in zip(gt, [k for k in range(len(sc["edges"])) if sc["truth"][k]])]
    s = pg.evaluate_refined_log(edge, gt, gt_info)
    assert s["recall"] == 1.0 and s["precision"] == 1.0 and not any(k.startswith("inlier_") for k in s)


@pytest.fixture(scope="module")
def scene():
    sc = fr.synthetic_scene(0, 6, 4000)
    F = len(sc["clouds"])
    M = max(len(x) for x in sc["xyz"])
    kp, de, cnt = np.zeros((F, 3, M), np.float32), np.zeros((F, sc["desc"][0].shape[1], M), np.float32), np.zeros(F, np.int32)
    for i in range(F):
        n = len(sc["xyz"][i])
        kp[i, :, :n], de[i, :, :n], cnt[i] = sc["xyz"][i].T, sc["desc"][i].T, n
    pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    return sc, kp, de, cnt, f1, f2, fr.host_bank(sc["clouds"]), fr.refine_bank_cpu(sc["clouds"])


def test_pipeline_prunes_a_planted_false_loop_closure(scene):
    sc, kp, de, cnt, f1, f2, bank, fine = scene
    args = (kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2], bank, f1, f2, np.arange(len(f1)))
    kw = dict(max_trials=3000, num_threads=16, refine=fine)
    plain = fr.register_pairs_cpu(*args, **kw)
    dense = fr.register_pairs_cpu(*args, dense_radius=pg.INFORMATION_RADIUS, **kw)
    assert list(dense)[:len(plain)] == list(plain) and list(dense)[len(plain):] == ["dense_information", "dense_count"]
    for k in plain:                                                    # every key returned without it is unchanged
        assert np.array_equal(bits(dense[k]), bits(plain[k])), k
    assert np.array_equal(dense["dense_information"][:, 0, 0], dense["dense_count"])
    ids = list(range(len(sc["clouds"])))
    gated = dense["gate_refined"].astype(bool)
    assert gated.sum() >= 5 and dense["dense_count"][gated].min() > 100
    # plant: a loop closure the gate refused enters the log with a pose that is far off
    planted = [p for p in range(len(f1)) if f2[p] - f1[p] > 1 and not gated[p]][0]
    false = {k: v.copy() for k, v in dense.items()}
    false["gate_refined"][planted] = True
    wrong = po.to4(false["refined_Rt"][planted]) @ po.disturb(np.random.default_rng(1), 0.8, 1.0)
    false["refined_Rt"][planted] = wrong[:3]
    false["dense_information"][planted] = dense["dense_information"][gated][0]
    before = fr.summarize({k: v.copy() for k, v in false.items()}, ids, sc["gt"], sc["gt_info"], None, "gate_refined", "refined_Rt")
    s = fr.summarize(false, ids, sc["gt"], sc["gt_info"], None, "gate_refined", "refined_Rt", {"iterations1": 16, "iterations2": 8})
    for k in before:
        if k not in ("per_pair", "entries", "errors"):
            assert before[k] == s[k] or (before[k] != before[k] and s[k] != s[k]), k
    assert set(s) - set(before) == {"loop_recall", "loop_precision", "loops_in", "loops_kept", "refined_entries", "split"}
    pp = s["per_pair"]
    assert pp["loop_status"][0] == 0 and pp["loop_kept"][planted] == 0 and pp["loop_weight"][planted] < 0.2
    true_loops = [p for p in range(len(f1)) if gated[p] and f2[p] - f1[p] > 1]
    assert all(pp["loop_kept"][p] == 1 and pp["loop_weight"][p] > 0.3 for p in true_loops)
    assert s["loops_in"] == len(true_loops) + 1 and s["loops_kept"] == len(true_loops)
    assert s["loop_precision"] >= s["precision"] and s["loop_precision"] == 1.0 and s["precision"] < 1.0
    print("precision %.3f -> %.3f, recall %.3f -> %.3f after pruning; the planted pair's weight %.2e"
          % (s["precision"], s["loop_precision"], s["recall"], s["loop_recall"], pp["loop_weight"][planted]))
    assert (int(f1[planted]), int(f2[planted])) not in [e.info[:2] for e in s["refined_entries"]]
    odom, odom_info, loop, loop_info = s["split"]
    assert [e.info[:2] for e in odom] == [(k, k + 1) for k in range(len(ids) - 1)] and len(loop) == s["loops_in"]
    # without the argument nothing of it appears; without the dense information it cannot run
    assert "loop_kept" not in fr.summarize(plain, ids, sc["gt"], sc["gt_info"], None, "gate_refined", "refined_Rt")["per_pair"]
    with pytest.raises(ValueError, match="dense_information"):
        fr.summarize(plain, ids, sc["gt"], sc["gt_info"], None, "gate_refined", "refined_Rt", {})
    with pytest.raises(ValueError, match="unknown keys"):
        fr.summarize(dense, ids, sc["gt"], sc["gt_info"], None, "gate_refined", "refined_Rt", {"tau": 1.0})
    with pytest.raises(ValueError, match="dense_radius needs refine"):
        fr.register_pairs_cpu(*args, max_trials=300, dense_radius=0.05)
    with pytest.raises(ValueError, match="needs refine=True"):
        fr.FragmentEvaluator(None, None, None, "cpu", optimize=True)


def test_fill_decides_what_stands_in_for_a_missing_odometry_pair(scene):
    sc, kp, de, cnt, f1, f2, bank, fine = scene
    pairs = list(zip(f1.tolist(), f2.tolist()))
    n = len(sc["clouds"])
    plan = pg.EdgePlan(pairs, n, "gt", sc["gt"], sc["gt_info"])
    assert plan.C == len(pairs) and plan.chain.tolist() == [pairs.index((k, k + 1)) for k in range(n - 1)]
    gate = np.zeros(len(pairs), bool)
    plan.check_chain(gate)                                             # gt fills every pair of the chain
    none = pg.EdgePlan(pairs, n, None)
    with pytest.raises(ValueError, match="lacks the pair \\(0, 1\\)"):
        none.check_chain(gate)
    pg.EdgePlan(pairs, n, "estimate").check_chain(gate)
    with pytest.raises(ValueError, match="lacks the pair \\(2, 3\\)"):
        pg.EdgePlan([p for p in pairs if p != (2, 3)], n, "estimate")
    with pytest.raises(ValueError, match="i < j"):
        pg.EdgePlan([(1, 0)], 2, None)


# ------------------------------------------------------------------------------------------------ the sanitised twin
SANITIZE = os.path.join(ROOT, "tests", "posegraph_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/posegraph_cpu.cpp: random graphs and banks with ids, counts and indices
    in and out of range.  It links nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "posegraph_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "posegraph_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
