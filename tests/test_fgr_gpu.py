"""The f-12 kernels on the MI355X (csrc/fgr.hip) against the library's host twin, which runs the same header
(csrc/fgr_math.h) with the trials as a sequential loop.  Device and twin are held to equality as bit patterns on every
output -- the mutual list, the normalisation, the accepted rows, the count of trials walked, the float64 estimate, the
inlier mask -- which is what proves the parallel walk a replay of the loop, the sums taken in the contract's order and
fgr_sincos the same function on both sides.  The twin itself is held to the numpy oracle in tests/test_fgr_cpu.py, whose
fixtures these are."""
import numpy as np
import pytest
import torch

import fgr_oracle as fo
import test_fgr_cpu as host
from usip_amd import fragments as fr
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def on_device(kp1, kp2, n1, n2, nn12, nn21, triples=None, seed=0, ids=None, want=0):
    d = [dev(a) for a in (kp1, kp2, n1, n2, nn12, nn21)]
    t = ops.fgr_tuples(*d, seed, None if ids is None else dev(ids), None if triples is None else dev(triples), want)
    o = ops.fgr_optimize(d[0], d[1], t["mutual"], t["mutual_count"], t["norm"], t["rows"], t["row_count"],
                         fr.INLIER_THRESHOLD)
    return {k: cpu(v) for k, v in {**t, **o}.items() if v is not None}


def on_host(kp1, kp2, n1, n2, nn12, nn21, triples=None, seed=0, ids=None, want=0):
    t = fr.fgr_tuples_cpu(kp1, kp2, n1, n2, nn12, nn21, seed, ids, triples, want, 16)
    o = fr.fgr_optimize_cpu(kp1, kp2, t["mutual"], t["mutual_count"], t["norm"], t["rows"], t["row_count"],
                            fr.INLIER_THRESHOLD, 16)
    return {k: v for k, v in {**t, **o}.items() if v is not None}


def same(got, want):
    assert set(got) == set(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (k, len(bad), bad[:5].tolist())
    return got


@pytest.mark.parametrize("name", fo.NAMES)
def test_fixture_equals_the_host_twin(name):
    arrays = host.batch([name])
    o = fo.fixture(name)["oracle"]
    got = same(on_device(*arrays), on_host(*arrays))                   # explicit triples
    assert int(got["mutual_count"][0]) == o["nc"] and int(got["row_count"][0]) == o["row_count"]
    assert int(got["trials_walked"][0]) == o["trials_walked"] and int(got["valid"][0]) == o["valid"]
    T = max(100 * o["nc"], 1)
    same(on_device(*arrays[:6], seed=3, want=T), on_host(*arrays[:6], seed=3, want=T))          # Philox draws


def test_ragged_batch_equals_the_host_twin():
    names = [n for n in fo.NAMES if n != "counts_beyond"]
    arrays = host.batch(names)
    got = same(on_device(*arrays), on_host(*arrays))
    for p, name in enumerate(names):
        o = fo.fixture(name)["oracle"]
        assert int(got["row_count"][p]) == o["row_count"] and int(got["trials_walked"][p]) == o["trials_walked"], name
        assert int(got["valid"][p]) == o["valid"] and int(got["inliers"][p]) == o["inliers"], name
    ids = np.arange(40, 40 + len(names), dtype=np.int64)
    same(on_device(*arrays[:6], seed=11, ids=ids, want=2000), on_host(*arrays[:6], seed=11, ids=ids, want=2000))


def test_counts_outside_the_range_behave_as_the_ends():
    kp1, kp2, n1, n2, nn12, nn21, triples = host.batch(["cap"])
    ref = on_device(kp1, kp2, n1, n2, nn12, nn21, triples)
    same(on_device(kp1, kp2, np.array([2 ** 31 - 1], np.int32), np.array([65], np.int32), nn12, nn21, triples), ref)
    none = same(on_device(kp1, kp2, n1, np.array([-3], np.int32), nn12, nn21, triples),
                on_host(kp1, kp2, n1, np.array([-3], np.int32), nn12, nn21, triples))
    assert int(none["mutual_count"][0]) == 0 and int(none["valid"][0]) == 0


def test_two_calls_and_a_side_stream_agree():
    arrays = host.batch(["cap", "sparse", "few_rows", "limit"])
    first = on_device(*arrays[:6], seed=5, want=1000)
    same(on_device(*arrays[:6], seed=5, want=1000), first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = on_device(*arrays[:6], seed=5, want=1000)
    torch.cuda.current_stream(DEV).wait_stream(side)
    same(third, first)


def test_shapes_outside_the_limits_are_refused():
    kp = torch.zeros((1, 3, 1025), dtype=torch.float32, device=DEV)
    z = torch.zeros((1, 1025), dtype=torch.int32, device=DEV)
    n = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        fr.fgr_registration(kp, kp, n, n, z, z)
    with pytest.raises(RuntimeError):
        fr.fgr_registration(kp[:, :, :16].contiguous().cpu(), kp[:, :, :16].contiguous().cpu(), n, n, z[:, :16], z[:, :16])


def scene_evaluator(sc, **kw):
    e = fr.FragmentEvaluator(None, None, None, DEV, top=128, **kw)
    for i in range(len(sc["clouds"])):
        e.add_fragment_result(i, sc["xyz"][i], sc["desc"][i], sc["clouds"][i])
    return e


def test_evaluator_with_fgr_equals_the_pipeline_of_host_twins_without_synchronising():
    sc = fr.synthetic_scene(0, 6, 4000)
    e = scene_evaluator(sc, batch_pairs=4, registrator="fgr")
    bank = e.bank()                                                       # uploads and the static sort: before the pairs
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        per_pair = e.evaluate_device()                                    # raises if anything synchronises
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
                                          bank.host(), f1[sl], f2[sl], np.arange(base, base + len(f1[sl])), num_threads=16,
                                          registrator="fgr"))
    want = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    same(got, want)
    s = fr.summarize(got, e.ids(), sc["gt"], sc["gt_info"])
    assert s["recall"] == 1.0 and s["gt_num"] >= 6
    full = e.evaluate(None, sc["gt"], sc["gt_info"])                      # the public call: the same numbers
    assert full["recall"] == 1.0 and full["pairs"] == 15 and np.array_equal(bits(full["per_pair"]["Rt"]), bits(got["Rt"]))


def test_ransac_through_the_new_argument_is_the_call_without_it():
    sc = fr.synthetic_scene(0, 4, 2000)
    a = scene_evaluator(sc, max_trials=300).evaluate_device()
    b = scene_evaluator(sc, max_trials=300, registrator="ransac").evaluate_device()
    assert list(a) == list(b)
    same({k: cpu(v) for k, v in b.items()}, {k: cpu(v) for k, v in a.items()})
    with pytest.raises(ValueError):
        fr.FragmentEvaluator(None, None, None, DEV, registrator="icp")
