"""The f-11 ISS kernels on the MI355X (csrc/iss.hip) against the library's host twin, which runs the same header
(csrc/iss_math.h) over ALL pairs of a frame, and against the independent oracle (tests/iss_oracle.py).  Device and host twin
are held to equality as bit patterns: the float64 saliency, the neighbour counts, the keypoint mask -- which is also what
proves the device's pruned walk exact and its sums taken in the contract's order.  Inputs and bars: tests/test_iss_cpu.py.

tiles_visited: a workgroup walks exactly the tiles of the x-sorted frame that intersect [xlo - rs, xhi + rs] (counted here in
numpy from the sorted x).  For the slab (2, 3000, 20) that is 2-3 of 12 tiles per workgroup; for (3, 3000, 3) 5-9 of 12 --
its x spans 6 > 2 + 2, so no workgroup can need all twelve; a frame whose x span is below rs (h = 0.9) takes all tiles."""
import os
import sys

import numpy as np
import pytest
import torch

import iss_oracle as io
import test_iss_cpu as host
from conftest import ROOT
from usip_amd import baselines as bl
from usip_amd import evaluation as ev
from usip_amd import fragments as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same_as_twin(pc, count=None, **kw):
    """pc [B,3,N] -> the device's (mask, saliency, neighbours) on the host, after the bit-for-bit comparison"""
    d = bl.iss_keypoints(dev(pc), None if count is None else dev(count), **kw)
    h = bl.iss_keypoints_cpu(pc, count, num_threads=16, **kw)
    d = tuple(cpu(t) for t in d)
    for name, a, b in zip(("mask", "saliency", "neighbours"), d, h):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (name, len(bad), bad[:5].tolist())
    return d


@pytest.mark.parametrize("name", sorted(host.golden.CASES))
def test_device_equals_the_bits_pinned_before_the_shared_walk(name):
    """tests/golden/make_baseline_walk_golden.py: what the host twin computed before csrc/ascending_walk.h held the kernels'
    body, every entry ==; on the five-tile case at radius 0.5 also the tiles each workgroup walked (the pruning still prunes)"""
    host.golden.check("iss", name, host.golden.iss_device(name, DEV), "device")


def test_ragged_batch_equals_the_host_twin():
    pc, count = host.ragged_batch()
    mask, sal, nb = same_as_twin(pc, count)
    assert mask[0].any() and mask[1].any()
    for b, n in enumerate(count):
        assert not mask[b, n:].any() and (sal[b, n:] == 0).all() and (nb[b, n:] == 0).all()


@pytest.mark.parametrize("inp", io.INPUTS)
def test_oracle_inputs_equal_the_host_twin_and_the_oracle(inp):
    pc = io.slab(*inp)
    got = same_as_twin(pc[None])
    o = host.against_oracle(host.one(got), pc)
    assert o["mask"].sum() == io.KEYPOINTS[inp]


@pytest.mark.parametrize("inp", [io.INPUTS[1], io.INPUTS[2]])
def test_two_radii(inp):
    pc = io.slab(*inp)
    got = same_as_twin(pc[None], salient_radius=2.0, non_max_radius=1.0)
    host.against_oracle(host.one(got), pc, salient_radius=2.0, non_max_radius=1.0)


def test_degenerate_and_small_frames():
    for name, pc in host.degenerate_frames().items():
        host.check_degenerate(name, *host.one(same_as_twin(pc[None])))
    for n in sorted(host.SMALL):
        pc = host.small_frame(n)
        host.against_oracle(host.one(same_as_twin(pc[None])), pc)


def tiles_expected(pc, rs):
    xs = np.sort(pc[0].astype(np.float64), kind="stable")
    n = len(xs)
    T = (n + 255) // 256
    lo, hi = xs[np.arange(T) * 256], xs[np.minimum(np.arange(T) * 256 + 255, n - 1)]
    return np.array([((lo[w] - hi < rs) & (lo - hi[w] < rs)).sum() for w in range(T)], np.int32)


def test_tiles_visited():
    frames = [io.slab(*inp) for inp in io.INPUTS] + [io.slab(3, 3000, 0.9)]
    for pc in frames:
        sal, nb, visits = bl.iss_saliency(dev(pc[None]), want_visits=True)
        want = tiles_expected(pc, 2.0)
        print(pc.shape[1], cpu(visits)[0].tolist())
        assert np.array_equal(cpu(visits)[0], want)
        hs, hn = bl.iss_saliency_cpu(pc[None], num_threads=16)
        assert np.array_equal(bits(cpu(sal)), bits(hs)) and np.array_equal(cpu(nb), hn)
    assert (tiles_expected(frames[2], 2.0) < 12).all()                   # (2, 3000, 20): every workgroup prunes
    assert tiles_expected(frames[3], 2.0).sum() > 2 * tiles_expected(frames[2], 2.0).sum()   # (3, 3000, 3): far less to prune
    assert (tiles_expected(frames[4], 2.0) == 12).all()                  # x span below rs: nothing to prune
    # a ragged batch: the workgroups without a live query walk nothing
    pc, count = host.ragged_batch()
    visits = cpu(bl.iss_saliency(dev(pc), dev(count), want_visits=True)[2])
    for b, n in enumerate(count):
        T = (n + 255) // 256
        assert np.array_equal(visits[b, :T], tiles_expected(pc[b, :, :n], 2.0)) and (visits[b, T:] == 0).all()


def test_wrong_permutations_and_arguments():
    """A permutation that does not sort, or leaves [0, n), gives wrong values (slots it never names stay unwritten) -- no
    read or write outside the frame: every entry is clamped into [0, n) before it is used."""
    pc = dev(io.slab(1, 1000, 12.0)[None])
    from usip_amd import ops
    for perm in (torch.arange(1000, dtype=torch.int32, device=DEV).flip(0).unsqueeze(0).contiguous(),
                 torch.full((1, 1000), 1 << 30, dtype=torch.int32, device=DEV),
                 torch.full((1, 1000), -7, dtype=torch.int32, device=DEV)):
        sal, nb = ops.iss_saliency(pc, None, perm, 2.0, 0.975, 0.975, 5)
        mask = ops.iss_nms(pc, None, perm, sal, 2.0, 5)
        assert sal.shape == nb.shape == mask.shape == (1, 1000)
    torch.cuda.synchronize()
    perm = bl.sort_along_x(pc)
    sal, nb = ops.iss_saliency(pc, None, perm, 2.0, 0.975, 0.975, 5)      # ... and the right one after them is right
    hs, hn = bl.iss_saliency_cpu(cpu(pc))
    assert np.array_equal(bits(cpu(sal)), bits(hs)) and np.array_equal(cpu(nb), hn)
    with pytest.raises(RuntimeError):
        ops.iss_saliency(pc.cpu(), None, perm, 2.0, 0.975, 0.975, 5)
    with pytest.raises(RuntimeError):
        ops.iss_saliency(pc, None, perm, 0.0, 0.975, 0.975, 5)
    with pytest.raises(RuntimeError):
        ops.iss_saliency(pc, None, perm, 2.0, 0.975, 0.975, 0)
    with pytest.raises(RuntimeError):
        ops.iss_nms(pc, None, perm.long(), torch.zeros(1, 1000, dtype=torch.float64, device=DEV), 2.0, 5)
    with pytest.raises(ValueError):
        bl.iss_keypoints(pc, non_max_radius=-1.0)


def test_selection_equals_the_twin():
    pc, mask, count = host.selection_case()
    for ensure in (True, False):
        d = bl.select_keypoints(dev(pc), dev(mask), dev(count), 16, ensure, 3, [5, 6, 7], want_index=True)
        h = bl.select_keypoints_cpu(pc, mask, count, 16, ensure, 3, [5, 6, 7], want_index=True)
        for a, b in zip(d, h):
            assert np.array_equal(cpu(a), b)
    d = bl.random_keypoints(dev(pc), dev(count), 64, 2, [0, 1, 2], want_index=True)
    h = bl.random_keypoints_cpu(pc, count, 64, 2, [0, 1, 2], want_index=True)
    for a, b in zip(d, h):
        assert np.array_equal(cpu(a), b)
    kp, cnt = bl.IssDetector(num=16, seed=3)(dev(pc), dev(count), [5, 6, 7])
    hm = bl.iss_keypoints_cpu(pc, count, num_threads=16)[0]
    hk, hc = bl.select_keypoints_cpu(pc, hm, count, 16, True, 3, [5, 6, 7])
    assert np.array_equal(cpu(kp), hk) and np.array_equal(cpu(cnt), hc)


def test_no_host_synchronisation_in_iss_keypoints():
    pc, count = host.ragged_batch()
    p, c = dev(pc), dev(count)
    bl.iss_keypoints(p, c)                                               # (the first call loads the code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = bl.iss_keypoints(p, c)                                     # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    h = bl.iss_keypoints_cpu(pc, count, num_threads=16)
    for a, b in zip(out, h):
        assert np.array_equal(bits(cpu(a)), bits(b))


def test_evaluators_take_baseline_keypoints():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 2, 4096)      # frame 1 = frame 0 moved by a known pose
    top, seed = 64, 2
    evaluator = ex.build_evaluator("ball", None, top=top, nms_radius=1.0, max_trials=500, seed=seed)
    ex.add_scans(evaluator, scans, nodes=128, seed=seed)
    learned = dict(evaluator.frames)
    ex.add_scans(evaluator, scans, nodes=128, seed=seed, method="iss")
    twin = {}
    for fid, rows in scans:
        pc = np.ascontiguousarray(rows.T[None, :3])
        m = bl.iss_keypoints_cpu(pc, num_threads=16)[0]
        twin[fid] = bl.select_keypoints_cpu(pc, m, None, top, True, seed, [fid])
        got, ref = evaluator.frames[fid], learned[fid]
        assert len(got) == len(ref) == 3
        for a, b in zip(got, ref):                                       # the layout add_frame caches
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and a.is_contiguous()
        assert np.array_equal(cpu(got[0]), twin[fid][0][0]) and int(got[2]) == int(twin[fid][1][0]) == top
        assert np.abs(np.linalg.norm(cpu(got[1]), axis=0) - 1).max() < 1e-3
    s = evaluator.evaluate(pairs)
    a, q, gt = pairs[0]
    want = ev.repeatability_cpu(twin[a][0], twin[a][1], twin[q][0], twin[q][1], np.asarray(gt)[None], 0.5)[0]
    assert s["per_pair"]["repeatability"][0] == want[0] and s["keypoint_num_mean"] == top
    # the indoor evaluator likewise
    fe = fr.FragmentEvaluator(None, evaluator.descriptor, evaluator.opt, DEV, top=top)
    fid, rows = scans[0]
    t = dev(rows.T)
    pc, sn = t[:3].unsqueeze(0).contiguous(), t[3:].unsqueeze(0).contiguous()
    kp, count = bl.IssDetector(num=top, seed=seed)(pc, None, [fid])
    got = fe.add_fragment_keypoints(fid, pc, sn, kp, count, rows[:, :3])
    assert len(got) == 4 and tuple(got[0].shape) == (3, top) and got[1].shape[1] == top and tuple(got[3].shape) == (4096, 3)
    assert np.array_equal(cpu(got[0]), twin[fid][0][0]) and torch.equal(got[1], evaluator.frames[fid][1])
