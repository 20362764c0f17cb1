"""f-14 on the device: the information kernel and the pose-graph optimiser of csrc/posegraph.hip against their host twins
(csrc/posegraph_cpu.cpp) BIT FOR BIT -- both sides run csrc/posegraph_math.h's operations in the same order -- on every
fixture of tests/posegraph_oracle.py, which tests/test_posegraph_cpu.py holds to the numpy restatement.  Then the evaluator:
FragmentEvaluator(refine=True, optimize=True) builds and optimises the scene's graph on the device without a host read, and
equals the pipeline of host twins key by key."""
import numpy as np
import pytest
import torch

import posegraph_oracle as po
import test_posegraph_cpu as host
from usip_amd import fragments as fr, ops, posegraph as pg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same(got, want):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (k, len(bad), bad[:5].tolist())
    return got


def optimize_both(scenes, it, **kw):
    b = po.batch_of(scenes)
    d = {k: dev(v) for k, v in b.items()}
    got = ops.posegraph_optimize(d["n"], d["ecount"], d["edge_i"], d["edge_j"], d["X"], d["info"], d["T0"], iterations1=it[0],
                                 iterations2=it[1], **kw)
    return {k: cpu(v) for k, v in got.items()}, pg.optimize_arrays_cpu(b, iterations1=it[0], iterations2=it[1], **kw)


@pytest.mark.parametrize("name", sorted(po.SCENES))
def test_fixture_equals_the_host_twin(name):
    sc = po.SCENES[name]()
    got, want = optimize_both([sc], po.ITERATIONS[name])
    same(got, want)
    assert got["status"][0] == 0 and np.array_equal(got["kept"][0, :len(sc["edges"])], sc["truth"])


def test_ragged_batch_equals_the_host_twin():
    scenes = [po.SCENES[n]() for n in ("12/14/8", "2/0/0", "half_y", "4/2/1")]
    got, want = optimize_both(scenes, (8, 3))
    same(got, want)
    for s, sc in enumerate(scenes):
        assert not got["T"][s, sc["n"]:].any() and not got["weight1"][s, len(sc["edges"]):].any()


def test_a_scene_that_ends_early_equals_the_host_twin():
    sc = dict(po.SCENES["4/2/1"]())
    keep = [k for k, (i, j) in enumerate(sc["edges"]) if 3 not in (i, j)]
    sc.update(edges=[sc["edges"][k] for k in keep], X=sc["X"][keep], L=sc["L"][keep])
    got, want = optimize_both([sc, po.SCENES["3/1/0"]()], (6, 2))
    same(got, want)
    assert got["status"].tolist() == [1, 0]


def test_two_calls_and_a_side_stream_agree():
    scenes = [po.SCENES[n]() for n in ("12/14/8", "third_111")]
    first, _ = optimize_both(scenes, (8, 3))
    same(optimize_both(scenes, (8, 3))[0], first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third, _ = optimize_both(scenes, (8, 3))
    torch.cuda.current_stream(DEV).wait_stream(side)
    same(third, first)


def test_information_equals_the_host_twin():
    clouds, pairs = po.information_bank()
    bank = fr.host_bank(clouds)
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    rng = np.random.default_rng(2)
    Rt = np.tile(np.eye(3, 4), (len(pairs), 1, 1))
    Rt[:7, :, 3] = rng.normal(size=(7, 3)) * 0.02
    Rt[13, :, 3] = 10.0
    mask = np.ones(len(pairs), np.uint8)
    mask[10] = 0
    rows, offsets, perm = dev(bank.rows), dev(bank.offsets), dev(bank.perm)
    idx, d2 = ops.icp_nearest(rows, offsets, perm, dev(f1), dev(f2), dev(Rt), bank.lmax, dev(mask))
    hidx, hd2 = fr.icp_nearest_cpu(bank, f1, f2, Rt, mask)
    same({"idx": cpu(idx), "d2": cpu(d2)}, {"idx": hidx, "d2": hd2})
    for radius in (0.12, po.LATTICE_RADIUS):
        info, count = ops.icp_information(rows, offsets, dev(f1), dev(f2), idx, d2, dev(mask), radius)
        hinfo, hcount = pg.icp_information_cpu(bank, f1, f2, hidx, hd2, mask, radius)
        same({"info": cpu(info), "count": cpu(count)}, {"info": hinfo, "count": hcount})
    assert cpu(count)[po.LATTICE_PAIR] == po.LATTICE_COUNT
    # the two-step wrapper, on a bank-like object
    class Bank:
        pass
    b = Bank()
    b.rows, b.offsets, b.perm, b.lmax = rows, offsets, perm, bank.lmax
    info, count = pg.dense_information(b, dev(f1), dev(f2), dev(Rt), dev(mask), 0.12)
    hinfo, hcount = pg.dense_information_cpu(bank, f1, f2, Rt, mask, 0.12)
    same({"info": cpu(info), "count": cpu(count)}, {"info": hinfo, "count": hcount})


def scene_evaluator(sc, **kw):
    e = fr.FragmentEvaluator(None, None, None, DEV, top=128, **kw)
    for i in range(len(sc["clouds"])):
        e.add_fragment_result(i, sc["xyz"][i], sc["desc"][i], sc["clouds"][i])
    return e


@pytest.mark.parametrize("registrator", ["ransac", "fgr"])
def test_evaluator_with_optimisation_equals_the_pipeline_of_host_twins_without_synchronising(registrator):
    sc = fr.synthetic_scene(0, 6, 4000)
    oargs = {"iterations1": 12, "iterations2": 4}
    e = scene_evaluator(sc, batch_pairs=4, registrator=registrator, max_trials=3000, refine=True, optimize=True,
                        optimize_args=oargs)
    bank, fine = e.bank(), e.refine_bank()                                # uploads, the grid and the static sorts: before the pairs
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        per_pair = e.evaluate_device(None, sc["gt"], sc["gt_info"])       # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = {k: cpu(v) for k, v in per_pair.items()}
    kp, de, cnt = [cpu(t) for t in e.stacked()]
    pairs = e.all_pairs()
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    want = []
    for base in range(0, len(pairs), 4):                                  # pair ids as the evaluator numbers them
        sl = slice(base, base + 4)
        want.append(fr.register_pairs_cpu(kp[f1[sl]], de[f1[sl]], cnt[f1[sl]], kp[f2[sl]], de[f2[sl]], cnt[f2[sl]],
                                          bank.host(), f1[sl], f2[sl], np.arange(base, base + len(f1[sl])), max_trials=3000,
                                          num_threads=16, registrator=registrator, refine=fine.host(),
                                          dense_radius=pg.INFORMATION_RADIUS))
    want = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    plan = pg.plan_for(pairs, e.ids(), sc["gt"], sc["gt_info"], oargs)
    want.update(pg.prune_pairs_cpu(plan, want["gate_refined"], want["Rt"], want["dense_information"], oargs))
    same(got, want)
    loops = (f2 - f1 > 1) & got["gate_refined"].astype(bool)
    assert got["loop_status"][0] == 0 and loops.any() and got["loop_kept"][loops].all()
    full = e.evaluate(None, sc["gt"], sc["gt_info"])                      # the public call
    assert full["loops_in"] == int(loops.sum()) == full["loops_kept"] and full["loop_precision"] >= full["precision"]
    assert len(full["refined_entries"]) == len(sc["clouds"]) - 1 + full["loops_kept"]
    plain = scene_evaluator(sc, batch_pairs=4, registrator=registrator, max_trials=3000, refine=True)
    off = scene_evaluator(sc, batch_pairs=4, registrator=registrator, max_trials=3000, refine=True, optimize=False)
    a, b = plain.evaluate_device(), off.evaluate_device()
    assert list(a) == list(b) and not set(pg.OPTIMIZE_KEYS) & set(b)
    same({k: cpu(v) for k, v in b.items()}, {k: cpu(v) for k, v in a.items()})
    same({k: got[k] for k in a}, {k: cpu(v) for k, v in a.items()})       # every key returned without it is unchanged
    assert "loop_recall" not in off.evaluate(None, sc["gt"], sc["gt_info"])


def test_limits_are_refused():
    sc = po.SCENES["4/2/1"]()
    d = {k: dev(v) for k, v in po.batch_of([sc]).items()}
    args = lambda **kw: [dict(d, **kw)[k] for k in ("n", "ecount", "edge_i", "edge_j", "X", "info", "T0")]
    for kw in (dict(tau2=0.0), dict(tau2=float("nan")), dict(prune=1.5), dict(iterations1=257), dict(iterations2=-1)):
        with pytest.raises(RuntimeError):
            ops.posegraph_optimize(*args(), **kw)
    with pytest.raises(RuntimeError):
        ops.posegraph_optimize(*args(), workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.posegraph_optimize(*args(T0=torch.zeros((1, 129, 3, 4), dtype=torch.float64, device=DEV)))
    with pytest.raises(RuntimeError):
        ops.posegraph_optimize(*args(X=d["X"].cpu()))
    with pytest.raises(RuntimeError):
        ops.posegraph_workspace_bytes(1, 4, 7)
    assert ops.posegraph_workspace_bytes(2, 57, 300) >= 2 * 336 * 336 * 8
    # a graph out of shape cannot be refused without reading the device: the scene gets status 4 and zeros, nothing is indexed
    bad_j = d["edge_j"].clone()
    bad_j[0, 0] = 1000
    unsorted_i, unsorted_j = d["edge_i"].flip(1).contiguous(), d["edge_j"].flip(1).contiguous()
    for kw in (dict(n=dev(np.array([9], np.int32))), dict(ecount=dev(np.array([-2], np.int32))), dict(edge_j=bad_j),
               dict(edge_i=unsorted_i, edge_j=unsorted_j)):
        o = {k: cpu(v) for k, v in ops.posegraph_optimize(*args(**kw), iterations1=2, iterations2=1).items()}
        assert o["status"].tolist() == [4] and not any(o[k].any() for k in o if k != "status")
    with pytest.raises(RuntimeError):
        pg.optimize([pg.build_graph(*host.graph_lists(sc))], tau2=-1.0, device=DEV)
    r, = pg.optimize([pg.build_graph(*host.graph_lists(sc))], iterations1=12, iterations2=4, device=DEV)
    w, = pg.optimize_cpu([pg.build_graph(*host.graph_lists(sc))], iterations1=12, iterations2=4)
    assert all(np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))) for a, b in zip(r, w))
