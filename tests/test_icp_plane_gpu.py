"""icp_fit_plane_kernel on the MI355X (csrc/icp_plane.hip) against the library's host twin, which
tests/test_icp_plane_cpu.py holds to the numpy oracle: device and twin are compared as BIT PATTERNS on every output of every
fixture under both settings -- Rt, iterations, converged, rmse, hits, ratio, the trim's cut (d2*, i*) of every pass and the 27
sums of every fit -- which is what proves the sums taken in the contract's lane-strided order, the tree the same in three
rounds of nine columns, the Cholesky solve and the step the twin's instructions.

Which mistake each fixture is for:
  lattice_*      exact sums: a row added twice or left out at the lane stride's tail (255, 256, 257 kept rows) or wrap (515)
                 changes a sum whatever the order; the bits of the oracle's sums are compared, not only the twin's.
  room_*         several rows per lane, iteration counts 1 to 9: a state not honoured between the launches, the pose read
                 before the step of the launch before, sums in another order (the bits of Rt).
  one_wall ..    a first, a last and an every pivot that is exactly zero: the pair must stop with the pose it came with, the
                 final pass must still run, and the NaNs of the abandoned solve must reach no output.
  empty_a ..     n1 = 0, n2 = 0, mask 0: the guards around empty ranges."""
import numpy as np
import pytest
import torch

import icp_oracle as io
import icp_plane_oracle as po
import test_icp_plane_cpu as host
from usip_amd import fragments as fr
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = po.bits
PLANE = host.PLANE


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


def refine_both(names, order="moved_x", **kw):
    """-> (device, twin): every output of the plane metric as numpy arrays"""
    bank, f1, f2, Rt0, mask = host.batch(names)
    args = dict(po.fixture(names[0])["args"])
    args.update(kw)
    ir, it, tt, tc, ar = fr._refine_args(args.get("inlier_ratio", fr.REFINE_INLIER_RATIO), args.get("max_iterations", fr.REFINE_ITERATIONS),
                                         args.get("tolerance", fr.REFINE_TOLERANCE), fr.REFINE_RADIUS)
    if order == "moved_x":
        order2 = fr.moved_x_order_cpu(bank, f2, Rt0)
    else:
        rng = np.random.default_rng(3)
        order2 = np.tile(np.arange(bank.lmax, dtype=np.int32), (len(names), 1))
        for p, name in enumerate(names):
            n2 = len(po.fixture(name)["B"])
            order2[p, :n2] = np.arange(n2)[::-1] if order == "reversed" else rng.permutation(n2)
    d = DeviceBank(bank)
    got = ops.icp_refine(d.rows, d.offsets, d.perm, dev(f1), dev(f2), dev(Rt0), bank.lmax, dev(mask), dev(order2), ir, it, tt,
                         tc, ar, want_cuts=True, want_sums=True, **PLANE)
    h, h_cut, h_i, h_sums = fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, num_threads=16, want_cuts=True, want_sums=True,
                                              order2=order2, **PLANE, **args)
    return {k: cpu(v) for k, v in got.items()}, {**h._asdict(), "cut_d2": h_cut, "cut_i": h_i, "fit_sums": h_sums}


def check_against_the_oracle(got, p, name, o):
    assert int(got["iterations"][p]) == o["iterations"] and int(got["converged"][p]) == o["converged"], name
    assert int(got["hits"][p]) == o["hits"], name
    if name in po.LATTICES:                                             # exact sums: the oracle's bits, whatever the order
        assert np.array_equal(bits(got["fit_sums"][p, 0]), bits(o["sums"][0])), name
    if name in po.FAILING or name in po.NOT_REFINED:
        assert np.array_equal(bits(got["Rt"][p]), bits(po.fixture(name)["Rt0"])), name
        assert np.isfinite(got["rmse"][p]) and np.isfinite(got["fit_sums"][p]).all(), name


@pytest.mark.parametrize("name", po.NAMES)
def test_fixture_equals_the_host_twin(name):
    got, want = refine_both([name])
    same(got, want)
    check_against_the_oracle(got, 0, name, po.fixture(name)["oracle"])


@pytest.mark.parametrize("name", po.TIGHT_NAMES)
def test_tight_setting_equals_the_host_twin(name):
    got, want = refine_both([name], **io.TIGHT)
    same(got, want)
    check_against_the_oracle(got, 0, name, po.tight(name))
    assert got["iterations"][0] <= 12 and not got["fit_sums"][0, got["iterations"][0]:].any()


def test_ragged_batch_equals_the_host_twin():
    names = list(host.RAGGED) + ["room_small"]
    got, want = refine_both(names, inlier_ratio=io.INLIER_RATIO, max_iterations=io.ITERATIONS)
    same(got, want)
    for p, name in enumerate(names):
        if name not in po.LATTICES:                                     # (those run under their own arguments elsewhere)
            check_against_the_oracle(got, p, name, po.fixture(name)["oracle"])


def test_the_order_of_the_queries_changes_no_answer():
    names = ["room_small", "lattice_515", "lattice_257", "two_walls"]
    kw = dict(inlier_ratio=1.0, max_iterations=4)
    sorted_, _ = refine_both(names, **kw)
    for order in ("reversed", "shuffled"):
        got, want = refine_both(names, order, **kw)
        same(got, want)
        same(got, sorted_)


def test_two_calls_and_a_side_stream_agree():
    names = ["room_small", "lattice_515", "masked", "one_wall"]
    kw = dict(inlier_ratio=io.INLIER_RATIO, max_iterations=io.ITERATIONS)
    first, _ = refine_both(names, **kw)
    same(refine_both(names, **kw)[0], first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third, _ = refine_both(names, **kw)
    torch.cuda.current_stream(DEV).wait_stream(side)
    same(third, first)


def test_negated_normals_change_no_bit_on_the_device():
    names = ["room_small", "lattice_plane", "two_walls"]
    kw = dict(inlier_ratio=io.INLIER_RATIO, max_iterations=io.ITERATIONS)
    want, _ = refine_both(names, **kw)
    bank, f1, f2, Rt0, mask = host.batch(names, flip=host.negate_half)
    r, cut_d2, cut_i, sums = fr.icp_refine(DeviceBank(bank), dev(f1), dev(f2), dev(Rt0), dev(mask), want_cuts=True,
                                           want_sums=True, **PLANE, **kw)
    same({**{k: cpu(v) for k, v in r._asdict().items()}, "cut_d2": cpu(cut_d2), "cut_i": cpu(cut_i), "fit_sums": cpu(sums)}, want)


def test_refine_bank_with_normals_equals_the_host_twin():
    clouds = list(io.fixture("room_small")["clouds"]) + [np.zeros((0, 3), np.float32), io.fixture("room_small")["clouds"][0][:6]]
    got, want = fr.RefineBank(clouds, DEV, normals=True), fr.refine_bank_cpu(clouds, normals=True)
    assert tuple(got.rows.shape) == want.rows.shape and want.rows.shape[1] == 6 and got.lmax == want.lmax
    same({"rows": cpu(got.rows), "offsets": cpu(got.offsets), "perm": cpu(got.perm)},
         {"rows": want.rows, "offsets": want.offsets, "perm": want.perm})
    plain = fr.RefineBank(clouds, DEV)                                  # the default builds the bank as before
    assert tuple(plain.rows.shape) == (want.rows.shape[0], 3) and torch.equal(plain.rows, got.rows[:, :3])
    with pytest.raises(ValueError):
        fr.icp_refine(plain, dev(np.zeros(1, np.int32)), dev(np.ones(1, np.int32)), dev(io.fixture("room_small")["Rt0"][None]),
                      **PLANE)
    with pytest.raises(ValueError):
        fr.icp_refine(got, dev(np.zeros(1, np.int32)), dev(np.ones(1, np.int32)), dev(io.fixture("room_small")["Rt0"][None]),
                      want_sums=True)


def scene_evaluator(sc, **kw):
    e = fr.FragmentEvaluator(None, None, None, DEV, top=128, **kw)
    for i in range(len(sc["clouds"])):
        e.add_fragment_result(i, sc["xyz"][i], sc["desc"][i], sc["clouds"][i])
    return e


@pytest.mark.parametrize("registrator", ["ransac", "fgr"])
def test_evaluator_under_the_plane_metric_equals_the_pipeline_of_host_twins_without_synchronising(registrator):
    sc = fr.synthetic_scene(0, 6, 4000)
    e = scene_evaluator(sc, batch_pairs=4, registrator=registrator, max_trials=300, refine=True, refine_metric="point_to_plane")
    bank, fine = e.bank(), e.refine_bank()                                # uploads, the grid, the normals, the static sorts
    assert fine.normals and fine.rows.shape[1] == 6
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
                                          num_threads=16, registrator=registrator, refine=fine.host(),
                                          refine_metric="point_to_plane"))
    want = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    same(got, want)
    assert got["gate_refined"].any() and got["refine_iterations"].max() >= 1


def test_the_default_metric_is_the_call_without_the_argument():
    sc = fr.synthetic_scene(0, 4, 2000)
    a = scene_evaluator(sc, max_trials=300, refine=True).evaluate_device()
    b = scene_evaluator(sc, max_trials=300, refine=True, refine_metric="point_to_point").evaluate_device()
    assert list(a) == list(b)
    same({k: cpu(v) for k, v in b.items()}, {k: cpu(v) for k, v in a.items()})
    c = scene_evaluator(sc, max_trials=300, refine=True, refine_metric="point_to_plane").evaluate_device()
    assert list(c) == list(a)                                           # the keys are the same under either metric
    names = ["room_small", "wall_255"]                                  # and icp_refine: f-13's fixtures, f-13's bits
    bank = fr.host_bank([x for n in names for x in (io.fixture(n)["A"], io.fixture(n)["B"])])
    f1, f2 = dev(np.array([0, 2], np.int32)), dev(np.array([1, 3], np.int32))
    Rt0 = dev(np.stack([io.fixture(n)["Rt0"] for n in names]))
    plain = fr.icp_refine(DeviceBank(bank), f1, f2, Rt0)
    named = fr.icp_refine(DeviceBank(bank), f1, f2, Rt0, metric="point_to_point")
    same({k: cpu(v) for k, v in named._asdict().items()}, {k: cpu(v) for k, v in plain._asdict().items()})
    with pytest.raises(ValueError):
        fr.FragmentEvaluator(None, None, None, DEV, refine=True, refine_metric="plane")
