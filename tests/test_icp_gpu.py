"""The f-13 kernels on the MI355X (csrc/icp.hip) against the library's host twin, whose nearest-neighbour search is the
plain loop over all rows.  Device and twin are held to equality as bit patterns on every output of every fixture and of the
ragged batch: for one nearest pass the neighbour and the float64 distance of every row, for the loop Rt, iterations,
converged, rmse, hits, ratio and the trim's cut (d2*, i*) of every pass -- which is what proves the tile walk exact, the radix select the same cut as the twin's
selection, and the fit's sums taken in the contract's order.  The twin itself is held to the numpy oracle in
tests/test_icp_cpu.py, whose fixtures these are.

Which mistake each fixture is for (tests/test_icp_cpu.py shows every one of them wrong on a numpy emulation of the walk):
  lattice        exact distances.  `>=` for `>` in the termination: a partner at exactly the best distance, with the lower
                 row index, sits in the first tile the bound would end the walk at, once to the left and once to the right;
                 a replacement test without the index tie-break: the same two queries and a three-way tie inside one tile;
                 the start tile's left neighbour skipped: one query's only near row lies there;
                 a trim that ignores the row index: the cut falls inside a run of 100 rows at d2 = 0, and i* itself is compared.
  wall_*         constant-x runs longer than a tile, 255 / 256 / 257 / 515 rows, fragment 2 below, beyond and on both sides:
                 the start tile's left neighbour skipped again (the answers lie in every tile), the binary search ending at
                 lo == n1 with the start tile clamped, a partial last tile read past its end.
  room_*         several workgroups and tiles, iteration counts 1, 4, 6 and the full 20: a state not honoured between the
                 launches, a history or a mean taken wrongly, sums in another order (the bits of Rt).
  one_row_a ..   n1 = 1, n2 = 1, m = max(1, 0), n1 = 0, n2 = 0, mask 0: the guards around empty ranges.
  coincident     every kept row on one point: the fit returns a finite pose, the identity rotation.
(Dropping `gap > 0` is not listed: it is implied by the strict bound, tests/test_icp_cpu.py has the argument.)"""
import numpy as np
import pytest
import torch

import icp_oracle as io
import test_icp_cpu as host
from usip_amd import fragments as fr
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same(got, want):
    assert set(got) == set(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (k, len(bad), bad[:5].tolist())
    return got


class DeviceBank:
    def __init__(self, bank):
        self.rows, self.offsets, self.perm, self.lmax = dev(bank.rows), dev(bank.offsets), dev(bank.perm), bank.lmax


def nearest_both(names, order="moved_x"):
    bank, f1, f2, Rt0, mask = host.batch(names)
    if order == "moved_x":
        order2 = fr.moved_x_order_cpu(bank, f2, Rt0)
    else:
        rng = np.random.default_rng(3)
        order2 = np.tile(np.arange(bank.lmax, dtype=np.int32), (len(names), 1))
        for p, name in enumerate(names):
            n2 = len(io.fixture(name)["B"])
            order2[p, :n2] = np.arange(n2)[::-1] if order == "reversed" else rng.permutation(n2)
    d = DeviceBank(bank)
    idx, d2, visits = ops.icp_nearest(d.rows, d.offsets, d.perm, dev(f1), dev(f2), dev(Rt0), bank.lmax, dev(mask), dev(order2),
                                      want_visits=True)
    h_idx, h_d2 = fr.icp_nearest_cpu(bank, f1, f2, Rt0, mask, order2, 16)
    return dict(idx=cpu(idx), d2=cpu(d2)), dict(idx=h_idx, d2=h_d2), cpu(visits)


def refine_both(names, **kw):
    bank, f1, f2, Rt0, mask = host.batch(names)
    args = dict(io.fixture(names[0])["args"])
    args.update(kw)
    d, d_cut, d_i = fr.icp_refine(DeviceBank(bank), dev(f1), dev(f2), dev(Rt0), dev(mask), want_cuts=True, **args)
    h, h_cut, h_i = fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, num_threads=16, want_cuts=True, **args)
    return ({**{k: cpu(v) for k, v in d._asdict().items()}, "cut_d2": cpu(d_cut), "cut_i": cpu(d_i)},
            {**h._asdict(), "cut_d2": h_cut, "cut_i": h_i})


@pytest.mark.parametrize("name", io.NAMES)
def test_fixture_equals_the_host_twin(name):
    got, want, visits = nearest_both([name])
    same(got, want)
    f = io.fixture(name)
    o = f["oracle"]
    if o["refined"]:
        n1, n2 = len(f["A"]), len(f["B"])
        print("%s: the walk evaluated %d of %d pairs" % (name, int(visits[0]), n1 * n2))
        first = io.nearest(f["A"], io.move(f["Rt0"], f["B"]))
        assert np.array_equal(got["idx"][0, :n2], first[0]) and np.array_equal(bits(got["d2"][0, :n2]), bits(first[1]))
    got, want = refine_both([name])
    same(got, want)
    assert int(got["iterations"][0]) == o["iterations"] and int(got["converged"][0]) == o["converged"]
    assert int(got["hits"][0]) == o["hits"]


@pytest.mark.parametrize("name", io.TIGHT_NAMES)
def test_tight_setting_equals_the_host_twin(name):
    got, want = refine_both([name], **io.TIGHT)
    same(got, want)
    assert int(got["iterations"][0]) == io.tight(name)["iterations"] >= 19


def test_ragged_batch_equals_the_host_twin():
    names = list(host.RAGGED) + ["coincident", "room_near"]
    same(*nearest_both(names)[:2])
    got, want = refine_both(names)
    same(got, want)
    for p, name in enumerate(names):
        o = io.fixture(name)["oracle"]
        if name != "coincident":                                        # (its own arguments; here it runs under the defaults)
            assert int(got["iterations"][p]) == o["iterations"] and int(got["hits"][p]) == o["hits"], name


def test_the_order_of_the_queries_changes_no_answer():
    names = ["room_small", "lattice", "wall_515", "wall_257"]
    sorted_, _, v0 = nearest_both(names)
    for order in ("reversed", "shuffled"):
        got, want, v = nearest_both(names, order)
        same(got, want)
        same(got, sorted_)
        print("%s: the walk evaluated %s pairs, %s with the queries sorted" % (order, v.tolist(), v0.tolist()))
    assert v0[0] < v[0]                                                 # the sort is what keeps the walk short


def test_two_calls_and_a_side_stream_agree():
    names = ["room_small", "wall_515", "masked", "lattice"]
    first, _ = refine_both(names)
    same(refine_both(names)[0], first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third, _ = refine_both(names)
    torch.cuda.current_stream(DEV).wait_stream(side)
    same(third, first)


def scene_evaluator(sc, **kw):
    e = fr.FragmentEvaluator(None, None, None, DEV, top=128, **kw)
    for i in range(len(sc["clouds"])):
        e.add_fragment_result(i, sc["xyz"][i], sc["desc"][i], sc["clouds"][i])
    return e


@pytest.mark.parametrize("registrator", ["ransac", "fgr"])
def test_evaluator_with_refinement_equals_the_pipeline_of_host_twins_without_synchronising(registrator):
    sc = fr.synthetic_scene(0, 6, 4000)
    e = scene_evaluator(sc, batch_pairs=4, registrator=registrator, max_trials=300, refine=True)
    bank, fine = e.bank(), e.refine_bank()                                # uploads, the grid and the static sorts: before the pairs
    assert same({"rows": fine.host().rows, "perm": fine.host().perm, "offsets": fine.host().offsets},
                dict(zip(("rows", "offsets", "perm"), fr.refine_bank_cpu(sc["clouds"])[:3])))
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
                                          bank.host(), f1[sl], f2[sl], np.arange(base, base + len(f1[sl])), max_trials=300,
                                          num_threads=16, registrator=registrator, refine=fine.host()))
    want = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    same(got, want)
    assert got["gate_refined"].any() and got["refine_iterations"].max() >= 1
    full = e.evaluate(None, sc["gt"], sc["gt_info"])                      # the public call: the refined gate, the estimate
    rows = np.nonzero(got["gate_refined"])[0]
    assert full["written"] == len(rows) and all(np.array_equal(en.trans[:3], got["Rt"][p]) for en, p in zip(full["entries"], rows))
    refined = scene_evaluator(sc, batch_pairs=4, registrator=registrator, max_trials=300, refine=True, log_transform="refined")
    full = refined.evaluate(None, sc["gt"], sc["gt_info"])
    assert all(np.array_equal(en.trans[:3], got["refined_Rt"][p]) for en, p in zip(full["entries"], rows))


def test_without_refinement_the_evaluator_is_the_call_without_the_argument():
    sc = fr.synthetic_scene(0, 4, 2000)
    a = scene_evaluator(sc, max_trials=300).evaluate_device()
    b = scene_evaluator(sc, max_trials=300, refine=False).evaluate_device()
    assert list(a) == list(b) and not set(fr.REFINE_KEYS) & set(b)
    same({k: cpu(v) for k, v in b.items()}, {k: cpu(v) for k, v in a.items()})
    with pytest.raises(ValueError):
        fr.FragmentEvaluator(None, None, None, DEV, log_transform="refined")
    with pytest.raises(ValueError):
        fr.FragmentEvaluator(None, None, None, DEV, refine=True, log_transform="icp")


def test_limits_are_refused():
    bank, f1, f2, Rt0, mask = host.batch(["one_row_b"])
    d = DeviceBank(bank)
    for kw in (dict(inlier_ratio=0.0), dict(max_iterations=65), dict(align_radius=0.0)):
        with pytest.raises(RuntimeError):
            fr.icp_refine(d, dev(f1), dev(f2), dev(Rt0), dev(mask), **kw)
    with pytest.raises(RuntimeError):
        ops.icp_refine(d.rows, d.offsets, d.perm, dev(f1), dev(f2), dev(Rt0), bank.lmax,
                       workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.icp_nearest(d.rows.cpu(), d.offsets, d.perm, dev(f1), dev(f2), dev(Rt0), bank.lmax)
    assert ops.icp_workspace_bytes(3, 1000) >= 3 * 1000 * 12


@pytest.mark.parametrize("name", io.NAMES)
def test_device_gives_the_pinned_parent_bits(name):
    """tests/golden/tile_walk_parent_bits.npz through icp_nearest_kernel over csrc/tile_walk.h: n = 1 and 0, a partial last
    tile, lo == n1 with the start tile clamped, constant-x runs longer than a tile."""
    host.tw.check("icp-" + name, host.tw.icp_device(name, DEV), "device")
