"""The f-13 host twin (csrc/icp_cpu.cpp over csrc/icp_math.h) against the numpy restatement of the contract
(tests/icp_oracle.py), on the smallest shapes at which each mechanism can go wrong.  tests/test_icp_gpu.py then holds the
device to this twin bit for bit.

Each fixture first passes the guards: no query's best and second-best d2, no cut of the trim, no convergence mean and no
distance against the alignment radius lies within 1e-9 (relative) of its decision -- except in the lattice fixture, whose
distances are exact and whose ties are the point.  Then the neighbours, the kept sets, iterations, converged and hits must be
EQUAL.  Rt and rmse: the oracle run with its kept rows forward and reversed differs from itself by its own summation noise
(measured over these fixtures: 2.2e-15); the twin, whose fit is a quaternion eigenvector where the oracle's is an SVD, may be
1000 times that away, and that allowance must itself stay below 1e-9 (error met: at most 4.3e-14, on the lattice whose
coordinates reach 80; 2.7e-15 elsewhere).

The mutants of the device's tile walk are checked here on the oracle's numpy emulation of it (icp_oracle.walk): each must
give a wrong neighbour on the fixture that exists for it, and the walk as written must equal the brute force everywhere.
Those three tests run the emulation only, no library code: icp_oracle.walk must be edited together with icp_nearest_kernel."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import icp_oracle as io
from conftest import GOLDEN, ROOT
from usip_amd import fragments as fr

sys.path.insert(0, GOLDEN)
import make_tile_walk_golden as tw  # noqa: E402   (the cases of tests/golden/tile_walk_parent_bits.npz and how they are stored)

MARGIN = 1e-9
POSE_IS_FREE = ("one_row_a",)       # every rotation about the one row fits equally well: the pose is not compared
EXACT = ("lattice", "lattice_round")  # exact distances and planted ties: no margin to guard
TIES_UNDER_A_ROUNDED_POSE = ("lattice_round",)      # the final pass after a fit: neighbours compared in "lattice" instead


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def batch(names):
    """the fixtures as one bank [A0, B0, A1, B1, ..] -> (bank, frag1, frag2, Rt0, mask)"""
    fx = [io.fixture(n) for n in names]
    bank = fr.host_bank([c for f in fx for c in (f["A"], f["B"])])
    P = len(fx)
    return (bank, np.arange(0, 2 * P, 2, dtype=np.int32), np.arange(1, 2 * P, 2, dtype=np.int32),
            np.stack([f["Rt0"] for f in fx]), np.array([f["mask"] for f in fx], np.uint8))


def twin(names, num_threads=4, **kw):
    bank, f1, f2, Rt0, mask = batch(names)
    args = dict(io.fixture(names[0])["args"])
    args.update(kw)
    return fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, num_threads=num_threads, want_neighbours=True, want_cuts=True, **args)


def allowance():
    noise = io.noise()
    print("oracle noise %.3e, allowance %.3e" % (noise, 1000 * noise))
    assert 0 < 1000 * noise < 1e-9
    return 1000 * noise


def guards(name, o):
    checks = ["stop_margin", "radius_margin"] + ([] if name in EXACT else ["nn_margin", "cut_margin"])
    for key in checks:
        assert o[key] > MARGIN, (name, key, o[key])


def against_oracle(res, p, name, o, allow):
    r, idx, d2, cut_d2, cut_i = res
    f = io.fixture(name)
    n2 = len(f["B"])
    guards(name, o)
    assert int(r.iterations[p]) == o["iterations"] and int(r.converged[p]) == o["converged"], (name, r.iterations[p])
    assert int(r.hits[p]) == o["hits"] and tuple(r.ratio[p]) == tuple(o["ratio"]), name
    if not o["refined"]:
        assert np.array_equal(bits(r.Rt[p]), bits(f["Rt0"])) and r.rmse[p] == 0 and not idx[p].any() and not d2[p].any(), name
        return
    assert not idx[p, n2:].any() and not d2[p, n2:].any(), name
    if name in POSE_IS_FREE:
        return
    if name not in TIES_UNDER_A_ROUNDED_POSE:
        assert np.array_equal(idx[p, :n2], o["idx"]), name
    # the twin's own cut (d2*, i*) of every pass, the final pass in the last column: the row the oracle's lexsort ends at,
    # and, for the final pass, the kept set it stands for
    slots = cut_i.shape[1]
    assert np.array_equal(cut_i[p, :len(o["cut_i"])], o["cut_i"]), (name, cut_i[p], o["cut_i"])
    assert not cut_i[p, len(o["cut_i"]):slots - 1].any() and not cut_d2[p, len(o["cut_i"]):slots - 1].any(), name
    assert name in TIES_UNDER_A_ROUNDED_POSE or int(cut_i[p, -1]) == o["final_cut_i"], (name, cut_i[p, -1], o["final_cut_i"])
    b, cut = bits(d2[p, :n2]), bits(cut_d2[p, -1:])[0]
    kept = np.nonzero((b < cut) | ((b == cut) & (np.arange(n2) <= cut_i[p, -1])))[0]
    assert len(kept) == io.trim_count(f["args"].get("inlier_ratio", io.INLIER_RATIO), n2), name
    assert name in TIES_UNDER_A_ROUNDED_POSE or np.array_equal(kept, o["kept"]), name
    err = max(float(np.abs(r.Rt[p] - o["Rt"]).max()), abs(float(r.rmse[p]) - o["rmse"]))
    print("%s: n1 %d, n2 %d, %d iterations, converged %d, hits %d, | Rt, rmse - oracle | %.3e" %
          (name, len(f["A"]), n2, o["iterations"], o["converged"], o["hits"], err))
    assert err <= allow, (name, err, allow)


@pytest.mark.parametrize("name", io.NAMES)
def test_fixture_equals_the_oracle(name):
    against_oracle(twin([name]), 0, name, io.fixture(name)["oracle"], allowance())


@pytest.mark.parametrize("name", io.TIGHT_NAMES)
def test_tight_setting_equals_the_oracle(name):
    o = io.tight(name)
    assert o["iterations"] >= 19
    against_oracle(twin([name], **io.TIGHT), 0, name, o, allowance())


@pytest.mark.parametrize("name", [n for n in io.NAMES if io.fixture(n)["oracle"]["refined"]])
def test_one_nearest_pass_carries_the_oracles_bits(name):
    bank, f1, f2, Rt0, _ = batch([name])
    f = io.fixture(name)
    idx, d2 = fr.icp_nearest_cpu(bank, f1, f2, Rt0)
    want_idx, want_d2, _ = io.nearest(f["A"], io.move(f["Rt0"], f["B"]))
    n2 = len(f["B"])
    assert np.array_equal(idx[0, :n2], want_idx) and np.array_equal(bits(d2[0, :n2]), bits(want_d2))
    tail, rng = np.arange(n2, bank.lmax, dtype=np.int32), np.random.default_rng(0)
    for head in (fr.moved_x_order_cpu(bank, f2, Rt0)[0, :n2], np.arange(n2, dtype=np.int32)[::-1], rng.permutation(n2)):
        again = fr.icp_nearest_cpu(bank, f1, f2, Rt0, order2=np.concatenate((head.astype(np.int32), tail))[None])
        assert np.array_equal(again[0], idx) and np.array_equal(bits(again[1]), bits(d2))


WALK_FIXTURES = ("lattice",) + tuple(io.WALLS) + ("room_small", "one_row_a", "one_row_b")


def emulated(name, **mutant):
    f = io.fixture(name)
    perm1 = np.argsort(f["A"][:, 0], kind="stable")
    q = io.move(f["Rt0"], f["B"])
    return io.walk(f["A"], perm1, q, np.argsort(q[:, 0], kind="stable"), **mutant), io.nearest(f["A"], q)


@pytest.mark.parametrize("name", WALK_FIXTURES)
def test_the_walk_as_written_equals_the_brute_force(name):
    (idx, d2, visited), (want_idx, want_d2, _) = emulated(name)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(d2), bits(want_d2))
    n1, n2 = len(io.fixture(name)["A"]), len(io.fixture(name)["B"])
    print("%s: %d of %d tile visits" % (name, visited, -(-n1 // io.TILE) * -(-n2 // io.TILE)))


@pytest.mark.parametrize("mutant,names", [(dict(strict=False), ("lattice",)), (dict(tiebreak=False), ("lattice",)),
                                          (dict(skip_left=True), ("lattice", "wall_257", "wall_515", "room_small"))])
def test_each_mutant_of_the_walk_fails_on_its_fixture(mutant, names):
    for name in names:
        (idx, _, _), (want_idx, _, _) = emulated(name, **mutant)
        wrong = np.nonzero(idx != want_idx)[0]
        print("%s under %s: %d wrong neighbours" % (name, mutant, len(wrong)))
        assert len(wrong) > 0, (name, mutant)
    if mutant in (dict(strict=False), dict(tiebreak=False)):            # the lattice: both directions of the walk
        f = io.fixture("lattice")
        (idx, _, _), (want_idx, _, _) = emulated("lattice", **mutant)
        x = f["queries"][:, 0]
        assert idx[x == 1000][0] != want_idx[x == 1000][0]              # the left plant
        if mutant == dict(strict=False):
            assert idx[x == 2000][0] != want_idx[x == 2000][0]          # the right plant
        else:
            assert idx[x == 3100][0] != want_idx[x == 3100][0]          # the three-way tie


@pytest.mark.parametrize("name", WALK_FIXTURES)
def test_dropping_the_sign_test_of_the_gap_changes_nothing(name):
    """`gap > 0` cannot be caught by any fixture: it is implied.  A direction's tile starts (ends) at x_e, and every row the
    lane has seen so far lies on the near side of x_e, so with the query beyond x_e (gap < 0) its best is at least (qx -
    x_e)^2 = gap gap and `gap gap > best` is false by itself; at gap = 0 it is false as well.  The condition stays in the code
    as the contract words it (it also keeps a NaN gap out); here the emulation shows the two forms agree, tile for tile."""
    (idx, d2, visited), _ = emulated(name)
    (idx_m, d2_m, visited_m), _ = emulated(name, gap_positive=False)
    assert np.array_equal(idx, idx_m) and np.array_equal(bits(d2), bits(d2_m)) and visited == visited_m


RAGGED = tuple(io.WALLS) + io.SMALL


def same_pair(a, pa, b, pb, width):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(bits(np.asarray(x)[pa]), bits(np.asarray(y)[pb]))
    for x, y in zip(a[3:], b[3:]):                                      # the cuts of every pass
        assert np.array_equal(bits(x[pa]), bits(y[pb]))
    for x, y in zip(a[1:3], b[1:3]):
        assert not x[pa, width:].any() and not y[pb, width:].any()
        assert np.array_equal(bits(x[pa, :width]), bits(y[pb, :width]))


def test_ragged_batch_equals_every_pair_alone_and_thread_counts_agree():
    whole = twin(list(RAGGED), num_threads=1)
    many = twin(list(RAGGED), num_threads=16)
    for p, name in enumerate(RAGGED):
        width = len(io.fixture(name)["B"])
        same_pair(whole, p, twin([name], num_threads=1), 0, width)
        same_pair(whole, p, many, p, width)
        against_oracle(whole, p, name, io.fixture(name)["oracle"], allowance())


def test_fragment_ids_and_counts_outside_the_bank_behave_as_the_ends():
    bank, f1, f2, Rt0, mask = batch(["wall_255", "one_row_b"])
    ref = fr.icp_refine_cpu(bank, f1, f2, Rt0, mask)
    got = fr.icp_refine_cpu(bank, [0, -7], [1, 99], Rt0[[0, 0]], mask)   # -7 -> fragment 0, 99 -> the last fragment
    assert np.array_equal(bits(got.Rt[0]), bits(ref.Rt[0])) and int(got.hits[0]) == int(ref.hits[0])
    want = fr.icp_refine_cpu(bank, [0], [3], Rt0[[0]], mask[[0]])
    assert np.array_equal(bits(got.Rt[1]), bits(want.Rt[0])) and int(got.iterations[1]) == int(want.iterations[0])


def test_refine_bank_equals_the_oracles_grid_average():
    clouds = list(io.fixture("room_small")["clouds"]) + [np.zeros((0, 3), np.float32)]
    bank = fr.refine_bank_cpu(clouds)
    assert bank.offsets.tolist() == [0, len(io.fixture("room_small")["A"]), bank.offsets[2], bank.offsets[2]]
    for k, want in enumerate((io.fixture("room_small")["A"], io.fixture("room_small")["B"])):
        got = bank.rows[bank.offsets[k]:bank.offsets[k + 1]]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        perm = bank.perm[bank.offsets[k]:bank.offsets[k + 1]]
        assert np.array_equal(perm, np.argsort(want[:, 0], kind="stable"))


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


@pytest.mark.parametrize("registrator", ["ransac", "fgr"])
def test_register_pairs_with_a_refine_bank_adds_keys_and_changes_none(scene, registrator):
    sc, kp, de, cnt, f1, f2, bank, fine = scene
    args = (kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2], bank, f1, f2, np.arange(len(f1)))
    kw = dict(max_trials=300, num_threads=16, registrator=registrator)
    plain = fr.register_pairs_cpu(*args, **kw)
    both = fr.register_pairs_cpu(*args, refine=fine, **kw)
    assert list(both)[:len(plain)] == list(plain) and tuple(list(both)[len(plain):]) == fr.REFINE_KEYS
    for k in plain:
        assert np.array_equal(bits(both[k]), bits(plain[k])), k
    assert not (both["gate_refined"] & ~(both["inlier_ratio"] > fr.GATE_INLIER_RATIO)).any()
    masked = ~((both["valid"] != 0) & (both["inlier_ratio"] > fr.GATE_INLIER_RATIO))
    assert not both["refine_iterations"][masked].any() and not both["refined_hits"][masked].any()
    assert np.array_equal(bits(both["refined_Rt"][masked]), bits(both["Rt"][masked]))
    assert both["gate_refined"].any() and both["refine_iterations"].max() >= 1
    print("%s: %d of %d pairs pass the first gate, %d the refined one" % (registrator, plain["gate"].sum(), len(f1),
                                                                        both["gate_refined"].sum()))
    # the four logs: either gate, either pose
    ids = list(range(len(sc["clouds"])))
    for gate in ("gate", "gate_refined"):
        for transform in ("Rt", "refined_Rt"):
            entries = fr.result_entries(both, ids, len(ids), gate, transform)
            rows = np.nonzero(both[gate])[0]
            assert [e.info[:2] for e in entries] == [(int(f1[p]), int(f2[p])) for p in rows]
            for e, p in zip(entries, rows):
                assert np.array_equal(e.trans[:3], both[transform][p]) and e.inlier_num == int(both["inliers"][p])
            s = fr.summarize(both, ids, sc["gt"], sc["gt_info"], None, gate, transform)
            assert s["written"] == len(rows) and s["pairs"] == len(f1) and s["good"] + s["bad"] + s["false_pos"] <= len(rows)
    assert [e.info for e in fr.result_entries(plain, ids, len(ids))] == [e.info for e in fr.result_entries(both, ids, len(ids))]
    with pytest.raises(KeyError):
        fr.result_entries(plain, ids, len(ids), "gate_refined")


def test_limits_are_refused():
    bank, f1, f2, Rt0, mask = batch(["one_row_b"])
    for kw in (dict(inlier_ratio=0.0), dict(inlier_ratio=1.5), dict(max_iterations=65), dict(max_iterations=-1),
               dict(tolerance=(-1.0, 0.009)), dict(align_radius=0.0)):
        with pytest.raises(RuntimeError):
            fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, **kw)
    with pytest.raises(ValueError):
        fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, tolerance=(0.01,))
    with pytest.raises(RuntimeError):
        fr.icp_refine_cpu(bank, np.zeros(65536, np.int32), np.ones(65536, np.int32), np.zeros((65536, 3, 4)))
    assert fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, max_iterations=0).iterations[0] == 0
    assert fr.chordal_tolerance(0.009) == io.chordal(0.009)


SANITIZE = os.path.join(ROOT, "tests", "icp_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# a host compiler: g++ or clang++ where there is one, otherwise the clang++ beside hipcc, which every build here needs anyway
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/icp_cpu.cpp: random banks, fragment ids, offsets, masks, orders and
    neighbour counts in and out of range.  It links nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "icp_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "icp_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout


@pytest.mark.parametrize("name", io.NAMES)
def test_twin_gives_the_bits_pinned_before_the_tile_walk_was_shared(name):
    """tests/golden/tile_walk_parent_bits.npz: one nearest pass (idx, d2) and every output of the loop, the cuts included,
    as the twin computed them before csrc/bank.h and csrc/host_split.h."""
    tw.check("icp-" + name, tw.icp_host(name), "host twin")
