"""f-18 on the host: the twins of csrc/ground_truth_cpu.cpp against getGtInfoLog.m restated in numpy (ground_truth_oracle.py),
the selection rule, the contract's refusals, the files, the end-to-end scoring and the repeatability pair list.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ground_truth_oracle as go
from conftest import ROOT
from usip_amd import _lib, fragments as fr, ground_truth as gtm


def truth_cpu(bank, c, cap=gtm.CAP, **kw):
    o = gtm.reach_cpu(bank, c["frag1"], c["frag2"], c["Rt"], mask=c.get("mask"), **kw)
    o["info"], o["order"] = gtm.correspondence_information_cpu(bank, c["frag1"], c["frag2"], c["Rt"], o["key"], o["hits"], cap,
                                                               want_order=True)
    return o


def scene_case(sc):
    f1, f2, trans = gtm.scene_pairs(sc["poses"])
    return dict(frag1=f1, frag2=f2, Rt=np.ascontiguousarray(trans[:, :3]), trans=trans)


# ------------------------------------------------------------------------------------------------ the seeded scene
def test_seeded_scene_matches_the_restatement_and_the_reference_rule_keeps_twelve_pairs():
    sc = go.seeded_scene()
    bank, c = fr.host_bank(sc["clouds"]), scene_case(go.seeded_scene())
    o = truth_cpu(bank, c, num_threads=8)
    assert go.check_pairs_against_restatement(bank, c["frag1"], c["frag2"], c["Rt"], o, o["info"]) == 0
    gt, gt_info, pp = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=None, num_threads=8)
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    left_out = {(0, 4): 0.232, (0, 5): 0.000, (1, 5): 0.201}
    assert [tuple(g.info) for g in gt] == [(i, j, 6) for i, j in pairs if (i, j) not in left_out]
    assert [tuple(g.info) for g in gt_info] == [tuple(g.info) for g in gt]
    ratio = {pair: pp["ratio"][k, 0] for k, pair in enumerate(pairs)}
    for pair, r in left_out.items():
        assert abs(ratio[pair] - r) < 5e-4
    assert min(r for pair, r in ratio.items() if pair not in left_out) > 0.41
    hits = {pair: tuple(pp["hits"][k]) for k, pair in enumerate(pairs)}
    assert hits[(0, 1)] == (3138, 3137) and hits[(0, 5)] == (1, 0)
    assert np.array_equal(pp["hits"], o["hits"]) and np.array_equal(pp["info"], o["info"])
    for g, gi in zip(gt, gt_info):
        k = pairs.index(tuple(g.info[:2]))
        assert np.array_equal(g.trans, np.linalg.inv(sc["poses"][g.info[0]]) @ sc["poses"][g.info[1]])
        assert np.array_equal(gi.mat, o["info"][k]) and np.array_equal(gi.mat, gi.mat.T)


def test_seeded_scene_at_the_reference_leaf_matches_the_restatement_on_the_averaged_rows():
    sc = go.seeded_scene()
    bank, c = fr.refine_bank_cpu(sc["clouds"], 0.01), scene_case(sc)
    assert all(0 < bank.offsets[f + 1] - bank.offsets[f] <= len(sc["clouds"][f]) for f in range(6))
    o = truth_cpu(bank, c, num_threads=8)
    assert go.check_pairs_against_restatement(bank, c["frag1"], c["frag2"], c["Rt"], o, o["info"]) == 0
    gt, gt_info, pp = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=0.01, num_threads=8, batch_pairs=4)
    assert np.array_equal(pp["hits"], o["hits"]) and np.array_equal(pp["info"], o["info"])
    assert np.array_equal(pp["ratio"], o["ratio"]) and len(gt) == int(pp["kept"].sum()) == len(gt_info)


# ------------------------------------------------------------------------------------------------ thresholds, tile edges
def test_classes_at_the_thresholds_are_the_constructed_ones():
    c = go.constructed_case()
    bank = fr.host_bank(c["clouds"])
    o = truth_cpu(bank, c)
    for p in range(5):
        n2 = len(c["clouds"][c["frag2"][p]])
        assert np.array_equal(o["cls"][p, :n2], c["expect"][p]), p
        assert o["hits"][p, 1] == c["near_counts"][p] == int((c["expect"][p] == 2).sum())
        assert o["hits"][p, 0] == int((c["expect"][p] >= 1).sum())
    assert go.check_pairs_against_restatement(bank, c["frag1"], c["frag2"], c["Rt"], o, o["info"], with_moved_rounding=True) == 0


def test_tile_edges_in_one_call_of_mixed_lengths_and_alone():
    c = go.tile_edge_case()
    bank = fr.host_bank(c["clouds"])
    assert bank.lmax == 600 and bank.lmax % 64 != 0
    o = truth_cpu(bank, c, num_threads=3)
    assert go.check_pairs_against_restatement(bank, c["frag1"], c["frag2"], c["Rt"], o, o["info"], mask=c["mask"],
                                              with_moved_rounding=True) == 0
    for p in c["zero_pairs"]:                                          # n1 = 0, n2 = 0, mask = 0
        assert not o["cls"][p].any() and not o["hits"][p].any() and not o["ratio"][p].any() and not o["info"][p].any()
        assert (o["key"][p] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert not o["hits"][24].any() and not o["hits"][25].any()                 # the box 12 m away
    assert tuple(o["hits"][26]) == (300, 300) and tuple(o["ratio"][26]) == (1.0, 1.0)  # duplicates
    crossed = o["hits"][:20].reshape(5, 4, 2)[1:, 1:]                  # both lengths >= 255: rows in either class
    assert (crossed[..., 1] > 0).all() and (crossed[..., 0] > crossed[..., 1]).all()
    assert o["hits"][23, 1] > 0 and o["hits"][27, 1] > 0               # one x for all of fragment 1 / of fragment 2
    assert ((o["key"] != np.uint64(0xFFFFFFFFFFFFFFFF)) == (o["cls"] == 2)).all()
    assert (o["key"][o["cls"] == 2] >> np.uint64(63) == 0).all()
    for p in (7, 19):                                                  # P = 1: the pair's own id keeps its keys
        one = {k: v[p:p + 1] for k, v in c.items() if k in ("frag1", "frag2", "Rt", "mask")}
        alone = gtm.reach_cpu(bank, one["frag1"], one["frag2"], one["Rt"], mask=one["mask"], pair_ids=[p])
        for k in ("cls", "hits", "ratio", "key"):
            assert np.array_equal(alone[k][0], o[k][p]), (p, k)


def test_prune_switch_and_thread_counts_do_not_change_a_bit():
    for c in (go.tile_edge_case(), go.constructed_case()):
        bank = fr.host_bank(c["clouds"])
        want = gtm.reach_cpu(bank, c["frag1"], c["frag2"], c["Rt"], mask=c.get("mask"), prune=True, num_threads=1)
        for prune, nt in ((False, 1), (True, 5), (False, 16)):
            got = gtm.reach_cpu(bank, c["frag1"], c["frag2"], c["Rt"], mask=c.get("mask"), prune=prune, num_threads=nt)
            for k in want:
                assert np.array_equal(got[k], want[k]), (prune, nt, k)
        i1 = gtm.correspondence_information_cpu(bank, c["frag1"], c["frag2"], c["Rt"], want["key"], want["hits"], num_threads=1)
        i7 = gtm.correspondence_information_cpu(bank, c["frag1"], c["frag2"], c["Rt"], want["key"], want["hits"], num_threads=7)
        assert np.array_equal(i1, i7)


# ------------------------------------------------------------------------------------------------ selection
def test_selection_keeps_the_smallest_keys_and_depends_on_seed_and_pair_id_only():
    c = go.constructed_case()
    bank = fr.host_bank(c["clouds"])
    sel = {k: v[1:] for k, v in c.items() if k in ("frag1", "frag2", "Rt")}        # near counts 6, 7, 8, 300
    ids = np.array([11, 12, 13, 14], np.int64)
    o = gtm.reach_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], seed=5, pair_ids=ids)
    assert [int(v) for v in o["hits"][:, 1]] == [6, 7, 8, 300]
    info7, order = gtm.correspondence_information_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], o["key"], o["hits"], 7,
                                                      want_order=True)
    full = gtm.correspondence_information_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], o["key"], o["hits"], 300)
    huge = gtm.correspondence_information_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], o["key"], o["hits"], 5000)
    assert order.shape == (4, 7)
    for p, n in enumerate((6, 7, 8, 300)):
        near = np.nonzero(o["cls"][p] == 2)[0]
        want = sorted(near, key=lambda r: (int(o["key"][p, r]), r))[:7]
        assert list(order[p, :min(n, 7)]) == want[:min(n, 7)]
        q = go.moved(go.fragment_rows(bank, sel["frag2"][p]), sel["Rt"][p])
        dq = go.moved_rounding(go.fragment_rows(bank, sel["frag2"][p]), sel["Rt"][p])
        ref7, bound7 = go.cov_mat(q[want], dq)
        assert (np.abs(info7[p] - ref7) <= bound7).all() and info7[p][0, 0] == min(n, 7)
        ref, bound = go.cov_mat(q[sorted(near, key=lambda r: (int(o["key"][p, r]), r))], dq)
        assert (np.abs(full[p] - ref) <= bound).all() and full[p][0, 0] == n
    assert np.array_equal(info7[:2], full[:2]) and not np.array_equal(info7[2:], full[2:])   # cap >= count changes nothing
    assert np.array_equal(full, huge)
    # the same (seed, pair id) gives the same keys whatever P and the batch split
    for p in range(4):
        one = gtm.reach_cpu(bank, sel["frag1"][p:p + 1], sel["frag2"][p:p + 1], sel["Rt"][p:p + 1], seed=5, pair_ids=ids[p:p + 1])
        assert np.array_equal(one["key"][0], o["key"][p])
    rev = gtm.reach_cpu(bank, sel["frag1"][::-1], sel["frag2"][::-1], sel["Rt"][::-1], seed=5, pair_ids=ids[::-1])
    assert np.array_equal(rev["key"][::-1], o["key"])
    whole = gtm.pairs_ground_truth_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], cap=7, seed=5, pair_ids=ids)
    for step in (1, 3):
        part = gtm.pairs_ground_truth_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], cap=7, seed=5, pair_ids=ids,
                                          batch_pairs=step)
        for k in whole:
            assert np.array_equal(part[k], whole[k]), (step, k)
    assert np.array_equal(whole["info"], info7)
    # another seed, or another pair id, selects other rows of the 300 but counts the same
    for other in (gtm.reach_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], seed=6, pair_ids=ids),
                  gtm.reach_cpu(bank, sel["frag1"], sel["frag2"], sel["Rt"], seed=5, pair_ids=ids + 100)):
        assert np.array_equal(other["hits"], o["hits"]) and np.array_equal(other["cls"], o["cls"])
        assert set(gtm.select_rows_cpu(other["key"], 7)[3]) != set(order[3])
    # the key is the documented Philox word (numpy's Philox increments the counter before it generates a block)
    row = int(np.nonzero(o["cls"][0] == 2)[0][-1])
    assert row >= 1
    block = np.random.Philox(key=np.array([5, 0x67745f6b6579], np.uint64), counter=np.array([row - 1, 0, 11, 0], np.uint64))
    assert int(block.random_raw(1)[0]) >> 1 == int(o["key"][0, row])


# ------------------------------------------------------------------------------------------------ refusals
def test_every_invalid_argument_is_refused():
    c = go.constructed_case()
    bank = fr.host_bank(c["clouds"])
    lib = _lib.lib()
    rows, offsets, perm = bank.rows, bank.offsets, bank.perm
    P, L = 5, bank.lmax
    f1, f2, Rt = c["frag1"], c["frag2"], np.ascontiguousarray(c["Rt"])
    cls, key, hits, ratio = np.zeros((P, L), np.uint8), np.zeros((P, L), np.uint64), np.zeros((P, 2), np.int32), np.zeros((P, 2))
    info, order, count = np.zeros((P, 6, 6)), np.zeros((P, 7), np.int32), np.zeros(P, np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None    # noqa: E731

    def reach(rows=rows, row_len=3, offsets=offsets, F=6, total=len(rows), perm=perm, f1=f1, f2=f2, Rt=Rt, P=P, L=L, far=0.03,
              near=0.006, cls=cls, hits=hits, ratio=ratio, key=key):
        return lib.usip_gt_reach_f32_cpu(p(rows), row_len, p(offsets), F, total, p(perm), p(f1), p(f2), p(Rt), None, P, L, far,
                                         near, 0, None, 1, p(cls), p(hits), p(ratio), p(key), 1)

    def information(rows=rows, row_len=3, offsets=offsets, F=6, total=len(rows), f2=f2, Rt=Rt, order=order, count=count, P=P, L=L,
                    cap=7, info=info):
        return lib.usip_gt_information_f32_cpu(p(rows), row_len, p(offsets), F, total, p(f2), p(Rt), p(order), p(count), P, L,
                                               cap, p(info), 1)

    assert reach() == 0 and information() == 0 and reach(P=0) == 0 and information(P=0) == 0
    nan = float("nan")
    for kw in (dict(rows=None), dict(offsets=None), dict(row_len=2), dict(F=0), dict(total=-1), dict(P=-1), dict(P=65536),
               dict(L=0), dict(L=(1 << 24) + 1), dict(far=0.006), dict(far=0.005), dict(near=0.0), dict(near=-1.0), dict(far=nan),
               dict(near=nan), dict(far=0.0, near=0.0), dict(perm=None), dict(f1=None), dict(f2=None), dict(Rt=None),
               dict(cls=None), dict(hits=None), dict(ratio=None), dict(key=None)):
        assert reach(**kw) == -1, kw
    for kw in (dict(rows=None), dict(offsets=None), dict(row_len=2), dict(F=0), dict(total=-1), dict(P=-1), dict(P=65536),
               dict(L=0), dict(L=(1 << 24) + 1), dict(cap=0), dict(cap=65537), dict(f2=None), dict(Rt=None), dict(order=None),
               dict(count=None), dict(info=None)):
        assert information(**kw) == -1, kw
    assert information(cap=65536, order=np.zeros((P, 65536), np.int32)) == 0
    with pytest.raises(ValueError, match="fragment 1 .*scan_voxel_keys"):
        gtm.check_voxel_range([np.zeros((4, 3), np.float32), np.array([[0, 0, 0], [0, 10486.0, 0]], np.float32)], 0.01)
    with pytest.raises(ValueError, match="fragment 0 .*scan_voxel_keys"):
        gtm.check_voxel_range([np.zeros(((1 << 20) + 1, 3), np.float32)], 0.01)
    gtm.check_voxel_range([np.array([[0, 0, 0], [0, 10485.0, 0]], np.float32)], 0.01)


# ------------------------------------------------------------------------------------------------ files, end to end
def test_pose_files_round_trip_and_written_ground_truth_reads_back(tmp_path):
    sc = go.seeded_scene()
    for i, T in enumerate(sc["poses"]):
        gtm.write_fragment_pose(str(tmp_path / ("cloud_bin_%d.info.txt" % i)), T, "seeded", 50 * i, 50 * i + 49)
    with open(str(tmp_path / "cloud_bin_2.info.txt")) as f:
        head = f.readline().split()
    assert head == ["seeded", "100", "149"]
    for i, T in enumerate(sc["poses"]):
        got = gtm.read_fragment_pose(str(tmp_path / ("cloud_bin_%d.info.txt" % i)))
        assert got.shape == (4, 4) and np.allclose(got, T, rtol=0, atol=5e-9 * np.abs(T).max())
    # the reference's own layout: a name row, then four tab-separated rows; anything after row 4 is not read
    path = str(tmp_path / "cloud_bin_9.info.txt")
    with open(path, "w") as f:
        f.write("7-scenes-redkitchen\t 0\t 49\t\n")
        f.write("1\t 0\t 0\t 0.5\t\n0\t 1\t 0\t -2\t\n0\t 0\t 1\t 3.25\t\n0\t 0\t 0\t 1\t\n9\t 9\t 9\t 9\t\n")
    want = np.eye(4)
    want[:3, 3] = (0.5, -2, 3.25)
    assert np.array_equal(gtm.read_fragment_pose(path), want)
    with open(path, "w") as f:
        f.write("name\n1 0 0 0\n")
    with pytest.raises(ValueError):
        gtm.read_fragment_pose(path)
    gt, gt_info, _ = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=None, num_threads=8)
    log, info = gtm.write_scene_ground_truth(str(tmp_path / "seeded-evaluation"), gt, gt_info)
    assert os.path.basename(log) == "gt.log" and os.path.basename(info) == "gt.info"
    back, back_info = fr.read_log(log), fr.read_info(info)
    assert [tuple(b.info) for b in back] == [tuple(g.info) for g in gt] == [tuple(b.info) for b in back_info]
    for b, g in zip(back, gt):
        assert np.allclose(b.trans, g.trans, rtol=0, atol=1e-8 * np.abs(g.trans).max())
    for b, g in zip(back_info, gt_info):
        assert np.allclose(b.mat, g.mat, rtol=0, atol=5.1e-9)


def test_true_transforms_score_full_recall_and_precision_against_the_scene_ground_truth():
    sc = go.seeded_scene()
    gt, gt_info, pp = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=None, num_threads=8)
    result = [fr.ResultEntry(g.info, g.trans, 100, 0.5, gi.mat) for g, gi in zip(gt, gt_info)]
    s = fr.evaluate_log(result, gt, gt_info)
    assert s["recall"] == 1.0 and s["precision"] == 1.0 and s["gt_num"] == sum(1 for g in gt if g.info[1] - g.info[0] > 1) == 7
    # a pair the rule left out is a false positive, a wrong transform is not good
    extra = result + [fr.ResultEntry((0, 5, 6), pp["trans"][4], 100, 0.5, np.eye(6))]
    assert fr.evaluate_log(extra, gt, gt_info)["precision"] == 7 / 8
    wrong = [r._replace(trans=np.eye(4)) if tuple(r.info[:2]) == (0, 2) else r for r in result]
    assert fr.evaluate_log(wrong, gt, gt_info)["recall"] == 6 / 7


# ------------------------------------------------------------------------------------------------ repeatability
def stacked_landmarks(sc):
    M = max(len(x) for x in sc["xyz"])
    kp, count = np.zeros((len(sc["xyz"]), 3, M), np.float32), np.array([len(x) for x in sc["xyz"]], np.int32)
    for f, x in enumerate(sc["xyz"]):
        kp[f, :, :len(x)] = x.T
    return kp, count


def test_repeatability_pairs_are_the_log_and_counts_match_pdist2():
    sc = go.seeded_scene()
    gt, _, _ = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=None, num_threads=8)
    pairs = gtm.repeatability_pairs(gt)
    assert [(a, b) for a, b, _ in pairs] == [tuple(g.info[:2]) for g in gt]
    assert all(np.array_equal(T, g.trans) for (_, _, T), g in zip(pairs, gt))
    kp, count = stacked_landmarks(sc)
    kp = kp + np.random.default_rng(3).normal(scale=0.03, size=kp.shape).astype(np.float32)    # so that not every one repeats
    ratio, hits = gtm.scene_repeatability_cpu(kp, count, gt, 0.05)
    assert len(ratio) == len(gt) == len(hits)
    for k, (a, b, T) in enumerate(pairs):
        anc = kp[a, :, :count[a]].T.astype(np.float64)
        pos = go.moved(kp[b, :, :count[b]].T, T)
        d = np.sqrt(((anc[:, None, :] - pos[None, :, :]) ** 2).sum(-1)).min(1)               # pdist2, 'smallest', 1
        assert np.abs(d - 0.05).min() > 1e-9
        assert hits[k] == int((d < 0.05).sum()) and ratio[k] == hits[k] / count[a]
    assert 0 < hits.sum() < count[[a for a, _, _ in pairs]].sum()


# ------------------------------------------------------------------------------------------------ sanitizers
SANITIZE = os.path.join(ROOT, "tests", "ground_truth_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# a host compiler: g++ or clang++ where there is one, otherwise the clang++ beside hipcc, which every build here needs anyway
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twins_run_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/ground_truth_cpu.cpp: the tile-edge and selection shapes with fragment
    ids, offsets, permutations, orders and counts in and out of range.  It links nothing of the package and is never loaded
    into Python."""
    exe = str(tmp_path / "ground_truth_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "ground_truth_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
