"""The f-6 evaluation kernels on the MI355X (csrc/registration.hip) against the numpy float64 oracle (tests/eval_oracle.py)
and against the library's host twins, which run the same header (csrc/registration_math.h): device and host twin agree on
every count and every discrete decision.  The issue allowed 1e-12 on Rt between the two (sqrt and division might round
differently); measured on the MI355X they are bit-identical on every hypothesis, refit and delta_t, so equality is what is
asserted.  Only atan2 rounds differently (delta_deg: 1.7e-18 degrees met, 1e-12 allowed).  Tolerances against the oracle:
tests/test_registration_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_oracle as eo
import test_registration_cpu as host
from conftest import ROOT
from usip_amd import evaluation as ev

pytestmark = pytest.mark.gpu
THR = host.THR
TWIN_DEG = 1e-12


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(x1, x2, count, **kw):
    kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    r = ev.ransac_registration(dev(x1), dev(x2), dev(count), **kw)
    return ev.RegistrationResult(*[None if t is None else t.cpu().numpy() for t in r])


def same_result(d, h, exact=False):
    for k in ("inliers", "inlier_mask", "trialcount", "valid", "chosen", "counts"):
        assert np.array_equal(getattr(d, k), getattr(h, k)), k
    for k in ("Rt", "delta_t", "delta_deg"):
        a, b = getattr(d, k), getattr(h, k)
        if a is None:
            assert b is None
            continue
        err = np.abs(a - b).max() if a.size else 0.0
        print("device vs host twin %s: max |diff| %.3e" % (k, err))
        assert (np.array_equal(a, b) if exact or k != "delta_deg" else err <= TWIN_DEG), k


@pytest.fixture(scope="module")
def batch():
    return eo.make_batch(20260, P=4, n=512, T=2000)


def test_per_trial_parity_on_explicit_triplets(batch):
    from usip_amd import ops
    x1, x2, count, gt, tri = batch
    T = tri.shape[1]
    counts, hyp, _ = ops.ransac_trials(dev(x1), dev(x2), dev(count), T, THR, triplets=dev(tri), want_hypotheses=True)
    counts, hyp = counts.cpu().numpy(), hyp.cpu().numpy()
    host.check_trials(counts, hyp, host.oracle_for(batch), "device")
    hc, hh, _ = ev.ransac_trials_cpu(x1, x2, count, T, THR, triplets=tri)
    err = np.abs(hyp - hh).max()
    print("device vs host twin hypotheses: max |diff| %.3e, bit-identical %s" % (err, np.array_equal(hyp, hh)))
    assert np.array_equal(counts, hc)                                   # on ALL trials
    assert np.array_equal(hyp, hh)


@pytest.mark.parametrize("name", sorted(host.STOP_CASES))
def test_stopping_rule_on_hand_made_counts(name):
    from usip_amd import ops
    scores, n, max_trials = host.STOP_CASES[name]
    T = len(scores)
    x1, x2, count, gt, tri = eo.make_batch(5, P=1, n=n, T=T)
    chosen, trialcount = eo.replay(scores, n, max_trials)
    o = ops.ransac_select(dev(x1), dev(x2), dev(count), dev(np.asarray(scores, np.int32)[None]), max_trials, THR,
                          triplets=dev(tri))
    assert (int(o["chosen"][0]), int(o["trialcount"][0])) == (chosen, trialcount), name


def test_stopping_rule_across_scan_chunks():
    """The device evaluates the rule 256 trials at a time: improvements and the exit on either side of a chunk edge."""
    from usip_amd import ops
    n = 512
    rng = np.random.default_rng(17)
    cases = []
    for at in (255, 256, 257, 511, 512, 700):
        s = rng.integers(0, 12, 1200)
        s[at] = 40                               # budget ~9 600 at 40 of 512: runs to max_trials
        cases.append((s, 1199))
        s2 = s.copy()
        s2[at] = 200                             # budget ~75: ends right after the improvement
        cases.append((s2, 1199))
        cases.append((s, at))                    # max_trials at the edge
    x1, x2, count, gt, tri = eo.make_batch(5, P=1, n=n, T=1200)
    for s, m in cases:
        chosen, trialcount = eo.replay(list(s), n, m)
        o = ops.ransac_select(dev(x1), dev(x2), dev(count), dev(s.astype(np.int32)[None]), m, THR, triplets=dev(tri))
        assert (int(o["chosen"][0]), int(o["trialcount"][0])) == (chosen, trialcount)


@pytest.mark.parametrize("name", sorted(host.rg.CASES))
def test_device_gives_the_bits_pinned_before_the_kernels_were_merged(name):
    """tests/golden/ransac_parent_bits.npz: A runs through the f-6 names, B (counts on either side of a chunk edge, beyond
    one chunk) through the f-9 names; the differing entries per field are printed before the assertion."""
    from usip_amd import ops
    rg = host.rg
    x1, x2, count, gt, ids, seed, large = rg.inputs(name)
    trials, select = (ops.ransac_trials_large, ops.ransac_select_large) if large else (ops.ransac_trials, ops.ransac_select)
    d = [dev(x1), dev(x2), dev(count)]
    out = trials(*d, rg.T, rg.THR, seed, dev(ids), want_hypotheses=True, want_triplets=True)
    o = select(*d, out[0], rg.MAX_TRIALS, rg.THR, seed, dev(ids), gt=None if gt is None else dev(gt))
    got = rg.collect([t.cpu().numpy() for t in out], {k: None if v is None else v.cpu().numpy() for k, v in o.items()})
    host.check_parent_bits(name, got, host.load_golden(os.path.basename(rg.PATH)), "device")


def test_end_to_end_on_explicit_triplets(batch):
    x1, x2, count, gt, tri = batch
    T = tri.shape[1]
    d = run(x1, x2, count, threshold=THR, max_trials=T - 1, triplets=tri, gt=gt)
    for p in range(len(count)):
        o = eo.ransacfit(x1[p], x2[p], THR, T - 1, tri[p], gt[p])
        assert (int(d.chosen[p]), int(d.trialcount[p])) == (o["chosen"], o["trialcount"])
        assert np.array_equal(np.nonzero(d.inlier_mask[p])[0], o["inliers"]) and d.valid[p] == 1
        assert np.abs(d.Rt[p][:, :3] - o["Rt"][:, :3]).max() <= host.TOL_R
        assert np.abs(d.Rt[p][:, 3] - o["Rt"][:, 3]).max() <= host.TOL_T
        assert abs(d.delta_t[p] - o["delta_t"]) <= host.TOL_T and abs(d.delta_deg[p] - o["delta_deg"]) <= host.TOL_DEG
    same_result(d, ev.ransac_registration_cpu(x1, x2, count, THR, T - 1, triplets=tri, gt=gt))
    dt, dd = ev.compare_transform(dev(gt), dev(d.Rt))
    assert np.array_equal(dt.cpu().numpy(), d.delta_t) and np.array_equal(dd.cpu().numpy(), d.delta_deg)


def test_edge_counts_degenerate_triplets_and_invalid_pairs():
    x1, x2, count, gt, tri = eo.make_batch(8, P=4, n=64, T=50, counts=[0, 2, 3, 4], nmax=64, inlier_share=1.0)
    d = run(x1, x2, count, threshold=THR, max_trials=49, triplets=tri, gt=gt)
    same_result(d, ev.ransac_registration_cpu(x1, x2, count, THR, 49, triplets=tri, gt=gt))
    assert d.valid.tolist() == [0, 0, 1, 1] and (d.delta_t[:2] == 3).all() and (d.delta_deg[:2] == 6).all()
    # degenerate triplets: finite, orthonormal
    from usip_amd import ops
    n, T = 16, 4
    a, b = np.zeros((3, 3, n), np.float32), np.zeros((3, 3, n), np.float32)
    a[0], b[0] = 1.5, -2.5
    line = np.linspace(-30, 30, n, dtype=np.float32)
    a[1], b[1] = np.stack((line, 2 * line, 0.5 * line)) + 1, np.stack((line, 2 * line, 0.5 * line))
    rng = np.random.default_rng(2)
    a[2], b[2] = rng.normal(size=(3, n)), rng.normal(size=(3, n))
    t4 = np.zeros((3, T, 3), np.int32)
    t4[:, :] = [[0, 1, 2], [3, 9, 15], [5, 5, 5], [7, 7, 2]]
    cnt = np.full(3, n, np.int32)
    counts, hyp, _ = ops.ransac_trials(dev(a), dev(b), dev(cnt), T, THR, triplets=dev(t4), want_hypotheses=True)
    hyp = hyp.cpu().numpy()
    assert np.isfinite(hyp).all() and np.abs(np.linalg.det(hyp[..., :3]) - 1).max() < 1e-9
    hc, hh, _ = ev.ransac_trials_cpu(a, b, cnt, T, THR, triplets=t4)
    assert np.array_equal(counts.cpu().numpy(), hc) and np.array_equal(hyp, hh)
    # no inlier set of three
    rng = np.random.default_rng(4)
    u1 = rng.uniform(-40, 40, size=(1, 3, 64)).astype(np.float32)
    u2 = rng.uniform(-40, 40, size=(1, 3, 64)).astype(np.float32)
    t1 = np.stack([rng.choice(64, 3, replace=False) for _ in range(40)]).astype(np.int32)[None]
    g1 = np.concatenate((np.eye(3), np.zeros((3, 1))), 1)[None]
    d = run(u1, u2, np.array([64], np.int32), threshold=1e-3, max_trials=39, triplets=t1, gt=g1)
    assert d.valid[0] == 0 and d.inlier_mask.sum() == 0 and (d.delta_t[0], d.delta_deg[0]) == (3.0, 6.0)
    assert d.trialcount[0] == 40


def test_ragged_batch_equals_one_by_one_and_ignores_nan_padding():
    cs = [512, 100, 37, 5]
    x1, x2, count, gt, tri = eo.make_batch(9, P=4, n=512, T=300, counts=cs, nmax=600)
    d = run(x1, x2, count, threshold=THR, max_trials=299, triplets=tri, gt=gt)
    n1, n2 = x1.copy(), x2.copy()
    for p, c in enumerate(cs):
        n1[p, :, c:] = np.nan
        n2[p, :, c:] = np.nan
    same_result(run(n1, n2, count, threshold=THR, max_trials=299, triplets=tri, gt=gt), d, exact=True)
    for p, c in enumerate(cs):
        one = run(x1[p:p + 1, :, :c], x2[p:p + 1, :, :c], count[p:p + 1], threshold=THR, max_trials=299,
                  triplets=tri[p:p + 1], gt=gt[p:p + 1])
        assert np.array_equal(one.Rt[0], d.Rt[p]) and np.array_equal(one.counts[0], d.counts[p])
        assert np.array_equal(one.inlier_mask[0], d.inlier_mask[p, :c]) and one.trialcount[0] == d.trialcount[p]
    same_result(d, ev.ransac_registration_cpu(x1, x2, count, THR, 299, triplets=tri, gt=gt))


@pytest.mark.parametrize("n", [3, 4, 5, 511, 512, 1000])
def test_philox_draws_equal_the_host_twin(n):
    from usip_amd import ops
    T = 3000
    x = np.zeros((3, 3, n), np.float32)
    cnt = np.full(3, n, np.int32)
    ids = np.array([7, 123456789012, 7], np.int64)
    _, _, d = ops.ransac_trials(dev(x), dev(x), dev(cnt), T, THR, seed=5, pair_ids=dev(ids), want_triplets=True)
    _, _, h = ev.ransac_trials_cpu(x, x, cnt, T, THR, seed=5, pair_ids=ids)
    d = d.cpu().numpy()
    assert np.array_equal(d, h)                                           # triplet for triplet
    assert d.min() >= 0 and d.max() < n and np.array_equal(d[0], d[2])
    assert (d[..., 0] != d[..., 1]).all() and (d[..., 0] != d[..., 2]).all() and (d[..., 1] != d[..., 2]).all()
    _, _, alone = ops.ransac_trials(dev(x[:1]), dev(x[:1]), dev(cnt[:1]), T, THR, seed=5, pair_ids=dev(ids[1:2]),
                                    want_triplets=True)
    assert np.array_equal(alone.cpu().numpy()[0], d[1])                   # not on P or the batch position


def test_registration_recovers_a_known_pose_with_philox_draws():
    from usip_amd import ops
    x1, x2, count, gt, _ = eo.make_batch(31, P=3, n=512, T=1)
    ids = np.array([0, 5, 9], np.int64)
    d = run(x1, x2, count, threshold=THR, max_trials=10000, seed=1, pair_ids=ids, gt=gt)
    print("delta_t", d.delta_t, "delta_deg", d.delta_deg, "inliers", d.inliers, "trials", d.trialcount)
    assert d.valid.all() and (d.delta_t < 0.1).all() and (d.delta_deg < 0.5).all() and (d.inliers >= 150).all()
    _, _, drawn = ops.ransac_trials(dev(x1), dev(x2), dev(count), 10001, THR, seed=1, pair_ids=dev(ids), want_triplets=True)
    drawn = drawn.cpu().numpy()
    for p in range(3):
        o = eo.ransacfit(x1[p], x2[p], THR, 10000, drawn[p], gt[p])
        assert (o["chosen"], o["trialcount"]) == (int(d.chosen[p]), int(d.trialcount[p]))
    same_result(run(x1, x2, count, threshold=THR, max_trials=10000, seed=1, pair_ids=ids, gt=gt), d, exact=True)
    same_result(d, ev.ransac_registration_cpu(x1, x2, count, THR, 10000, seed=1, pair_ids=ids, gt=gt, num_threads=8))
    # the explicit path on the drawn triplets is the Philox path
    same_result(run(x1, x2, count, threshold=THR, max_trials=10000, triplets=drawn, gt=gt), d, exact=True)


def test_repeatability_against_oracle_and_host_twin():
    rng = np.random.default_rng(6)
    P, Ma, Mp = 5, 300, 1300                                    # more positives than one LDS chunk holds
    na, npos = np.array([300, 17, 0, 128, 64], np.int32), np.array([1300, 1025, 40, 0, 1], np.int32)
    pos = rng.uniform(-40, 40, size=(P, 3, Mp)).astype(np.float32)
    gt = np.stack([np.concatenate((eo.random_rotation(rng, 0.4), rng.uniform(-3, 3, size=(3, 1))), 1) for _ in range(P)])
    anc = np.full((P, 3, Ma), np.nan, np.float32)
    for p in range(P):
        m = min(na[p], npos[p])
        moved = gt[p][:, :3] @ pos[p].astype(np.float64) + gt[p][:, 3:4]
        anc[p, :, :na[p]] = rng.uniform(-40, 40, size=(3, na[p]))
        anc[p, :, :m] = moved[:, -m:] + rng.normal(0, 0.4, size=(3, m)) if m else anc[p, :, :m]
    for p in range(P):
        pos[p, :, npos[p]:] = np.nan
    ratio, hits, md = [t.cpu().numpy() for t in ev.repeatability(dev(anc), dev(na), dev(pos), dev(npos), dev(gt), 0.5)]
    near = 0
    for p in range(P):
        m, h, r = eo.repeatability(anc[p][:, :na[p]], pos[p][:, :npos[p]], gt[p], 0.5)
        near += int((np.abs(m - 0.5) < 1e-7).sum())
        if npos[p] and na[p]:
            assert np.abs(md[p, :na[p]] - m).max() <= 1e-9
        assert hits[p] == h and ratio[p] == r
    assert near == 0 and 0.2 < ratio[0] < 0.9
    hr, hh, hm = ev.repeatability_cpu(anc, na, pos, npos, gt, 0.5)
    assert np.array_equal(hits, hh) and np.array_equal(ratio, hr) and np.array_equal(md, hm)


def test_descriptor_matching_against_oracle_host_twin_and_dense_kernel():
    from usip_amd import ops
    rng = np.random.default_rng(12)
    B, C, M = 8, 128, 512
    anc, pos = host.unit_descriptors(rng, B, C, M), host.unit_descriptors(rng, B, C, M)
    full = np.full(B, M, np.int32)
    idx = ev.match_descriptors(dev(anc), dev(pos), dev(full), dev(full)).cpu().numpy()
    host.check_matches(idx, anc, pos, full, full)
    dd, da = ops.nearest_nd(dev(anc), dev(pos))
    cd, ca = ops.nearest_nd_counted(dev(anc), dev(pos), dev(full), dev(full))
    assert torch.equal(da, ca) and torch.equal(dd, cd)                     # the dense kernel, bit for bit
    na = np.array([512, 1, 0, 300, 77, 512, 64, 9], np.int32)
    nb = np.array([512, 400, 30, 1, 65, 129, 64, 500], np.int32)
    a2, p2 = anc.copy(), pos.copy()
    for p in range(B):
        a2[p, :, na[p]:] = np.nan
        p2[p, :, nb[p]:] = np.nan
    cd, ca = ops.nearest_nd_counted(dev(a2), dev(p2), dev(na), dev(nb))
    idx = ca.cpu().numpy()
    host.check_matches(idx, anc, pos, na, nb)
    assert np.array_equal(idx, ev.match_descriptors_cpu(a2, p2, na, nb))
    for p in range(B):                                                     # ragged against per-frame dense
        if na[p]:
            d1, a1 = ops.nearest_nd(dev(anc[p:p + 1, :, :na[p]]), dev(pos[p:p + 1, :, :nb[p]]))
            assert torch.equal(a1[0], ca[p, :na[p]]) and torch.equal(d1[0], cd[p, :na[p]])
    # first index on exact ties
    a, q = host.unit_descriptors(rng, 1, 32, 40), host.unit_descriptors(rng, 1, 32, 200)
    q[0, :, 150], q[0, :, 199] = q[0, :, 20], q[0, :, 70]
    a[0, :, 3], a[0, :, 4] = q[0, :, 20], q[0, :, 199]
    t = ev.match_descriptors(dev(a), dev(q), dev(np.array([40], np.int32)), dev(np.array([200], np.int32)))
    assert int(t[0, 3]) == 20 and int(t[0, 4]) == 70


def test_device_entries_refuse_host_tensors():
    x = torch.zeros(1, 3, 8)
    c = torch.full((1,), 8, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ev.ransac_registration(x, x, c, max_trials=10)
    with pytest.raises(RuntimeError):
        ev.ransac_registration(x.cuda(), x.cuda(), c)                      # a host count next to device points
    with pytest.raises(RuntimeError):
        ev.match_descriptors(x, x, c, c)
    with pytest.raises(RuntimeError):
        ev.repeatability(x, c, x, c, torch.zeros(1, 3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ev.ransac_registration(torch.zeros(1, 3, 2000).cuda(), torch.zeros(1, 3, 2000).cuda(), c.cuda())   # Nmax > 1024


def test_evaluator_reproduces_the_oracle_on_its_own_cached_frames(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    from usip_amd import inference
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 3, 4096)
    evaluator = ex.build_evaluator("ball", None, top=64, nms_radius=1.0, max_trials=500, seed=2)
    ex.add_scans(evaluator, scans, nodes=128, seed=2)
    s = evaluator.evaluate(pairs)
    for k in ("wrong", "inlier_ratio_mean", "trial_count_mean", "rte_mean", "rte_std", "rre_mean", "rre_std",
              "repeatability_mean", "repeatability_min", "repeatability_max", "keypoint_num_mean", "per_pair"):
        assert k in s
    per = s["per_pair"]
    for i, (a, q, gt) in enumerate(pairs):
        axyz, adesc = evaluator.frame_arrays(a)
        qxyz, qdesc = evaluator.frame_arrays(q)
        assert per["keypoint_num"][i] == len(axyz) and np.abs(np.linalg.norm(adesc, axis=1) - 1).max() < 1e-3
        arg, two = eo.match(adesc.T, qdesc.T)
        clear = (two[:, 1] - two[:, 0]) >= 1e-5 * two[:, 1]
        assert np.array_equal(per["match_idx"][i][:len(axyz)][clear], arg[clear])
        m, h, r = eo.repeatability(axyz.T, qxyz.T, np.asarray(gt), 0.5)
        assert per["repeatability"][i] == r
        # the same matches and the same draws through the oracle
        idx = per["match_idx"][i][:len(axyz)]
        x1, x2 = np.ascontiguousarray(axyz.T), np.ascontiguousarray(qxyz[idx].T)
        _, _, drawn = ev.ransac_trials_cpu(x1[None], x2[None], np.array([len(axyz)], np.int32), 501, 1.0, seed=2,
                                           pair_ids=np.array([i], np.int64))
        o = eo.ransacfit(x1, x2, 1.0, 500, drawn[0], np.asarray(gt))
        assert per["trialcount"][i] == o["trialcount"] and per["inliers"][i] == len(o["inliers"])
        assert bool(per["valid"][i]) == o["valid"]
        assert abs(per["delta_t"][i] - o["delta_t"]) <= host.TOL_T and abs(per["delta_deg"][i] - o["delta_deg"]) <= host.TOL_DEG
    again = ev.summarize({k: v for k, v in per.items()})
    assert again["wrong"] == s["wrong"] and again["repeatability_mean"] == s["repeatability_mean"]
    # a frame's descriptors do not depend on the call
    before = evaluator.frame_arrays(pairs[0][0])
    ex.add_scans(evaluator, scans[:1], nodes=128, seed=2)
    after = evaluator.frame_arrays(pairs[0][0])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    path = str(tmp_path / "f.bin")
    inference.write_descriptors_bin(path, *before)
    x, d = inference.read_descriptors_bin(path, 3 + before[1].shape[1])
    assert np.array_equal(x, before[0]) and np.array_equal(d, before[1])


def test_example_runs_end_to_end_and_prints_one_json_line(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "evaluate_registration.py"), "--make-synthetic",
                          str(tmp_path / "data"), "--frames", "3", "--points", "4096", "--nodes", "128", "--top", "64",
                          "--max-trials", "500", "--write-descriptors", str(tmp_path / "desc")],
                         check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    s = json.loads(lines[0])
    assert s["pairs"] == 2 and "repeatability_mean" in s and "rte_mean" in s and "wrong" in s
    assert len(os.listdir(str(tmp_path / "desc"))) == 3
