"""The f-16 Harris3D kernels on the MI355X (csrc/harris.hip) against the library's host twin, which runs the same header
(csrc/harris_math.h) over ALL pairs of a frame, and against the independent oracle (tests/harris_oracle.py).  Device and host
twin are held to equality as bit patterns: the float64 normals and responses, the neighbour and member counts, the keypoint
mask -- which is also what proves the device's pruned walk exact and its sums taken in the contract's order.  Inputs and bars:
tests/test_harris_cpu.py.  No shape is larger than B = 3, N = 3000.

tiles_visited: a workgroup walks exactly the tiles of the x-sorted frame that intersect [xlo - r, xhi + r] (counted here in
numpy from the sorted x)."""
import os
import sys

import numpy as np
import pytest
import torch

import harris_oracle as ho
import test_harris_cpu as host
from conftest import ROOT
from usip_amd import baselines as bl
from usip_amd import evaluation as ev
from usip_amd import fragments as fr
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits
NAMES = ("mask", "response", "members", "normals", "neighbours")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same_as_twin(pc, count=None, normals=None, **kw):
    """pc [B,3,N] -> the device's (mask, response, members, normals) and neighbours (None with supplied normals) on the host,
    after the bit-for-bit comparison"""
    d = bl.harris_keypoints(dev(pc), dev(count), normals=dev(normals), **kw)
    h, hnb = host.twin(pc, count, num_threads=16, normals=normals, **kw)
    d = tuple(cpu(t) for t in d)
    dnb = None
    if normals is None:
        dn, dnb = bl.harris_normals(dev(pc), dev(count), kw.get("radius", 1.0), kw.get("min_neighbors", 3))
        dnb = cpu(dnb)
        assert np.array_equal(bits(cpu(dn)), bits(d[3]))
    for name, a, b in zip(NAMES, d + (dnb,), h + (hnb,)):
        if a is None and b is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, name
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (name, len(bad), bad[:5].tolist())
    return d, dnb


@pytest.mark.parametrize("name", sorted(host.golden.CASES))
def test_device_equals_the_bits_pinned_before_the_shared_walk(name):
    """tests/golden/make_baseline_walk_golden.py: what the host twin computed before csrc/ascending_walk.h held the kernels'
    body, every entry ==; on the five-tile case at radius 0.5 also the tiles each workgroup walked (the pruning still prunes)"""
    host.golden.check("harris", name, host.golden.harris_device(name, DEV), "device")


def test_ragged_batch_equals_the_host_twin():
    pc, count = host.ragged_batch()
    (mask, res, members, normals), nb = same_as_twin(pc, count)
    assert mask[0].any() and mask[1].any()
    for b, n in enumerate(count):
        assert not mask[b, n:].any() and (res[b, n:] == 0).all() and (members[b, n:] == 0).all()
        assert (normals[b, :, n:] == 0).all() and (nb[b, n:] == 0).all()


@pytest.mark.parametrize("inp", ho.INPUTS)
def test_oracle_inputs_equal_the_host_twin_and_the_oracle(inp):
    pc = ho.boxes(*inp)
    got, nb = same_as_twin(pc[None])
    o = host.against_oracle(host.one(got), host.oracle(inp), nb[0])
    assert o["mask"].sum() == ho.KEYPOINTS[inp]


@pytest.mark.parametrize("response", ho.METHODS)
def test_every_response(response):
    inp = ho.INPUTS[1]
    got, _ = same_as_twin(ho.boxes(*inp)[None], response=response)
    host.against_oracle(host.one(got), host.oracle(inp, response))


def test_supplied_normals():
    for inp in ho.INPUTS[:3]:
        pc, analytic = ho.boxes(*inp, want_normals=True)
        got, _ = same_as_twin(pc[None], normals=analytic[None])
        host.against_oracle(host.one(got), host.oracle(inp, supplied=True))
    pc, nrm = host.noisy_normals(ho.INPUTS[3])
    nrm[:, 7] = 0.0
    nrm[1, 8] = np.nan
    nrm[2, 9] = np.inf
    got, _ = same_as_twin(pc[None], normals=nrm[None])
    host.against_oracle(host.one(got), ho.harris(pc, normals=nrm))
    assert (got[1][0, 7:10] == 0).all() and (got[2][0, 7:10] == 0).all()


def test_degenerate_and_small_frames():
    for name, pc in host.degenerate_frames().items():
        got, nb = same_as_twin(pc[None])
        host.check_degenerate(name, pc, *host.one(got), nb[0])
    for n in sorted(host.SMALL):
        pc = host.small_frame(n)
        got, nb = same_as_twin(pc[None])
        host.against_oracle(host.one(got), ho.harris(pc), nb[0])


def tiles_expected(pc, r):
    xs = np.sort(pc[0].astype(np.float64), kind="stable")
    n = len(xs)
    T = (n + 255) // 256
    lo, hi = xs[np.arange(T) * 256], xs[np.minimum(np.arange(T) * 256 + 255, n - 1)]
    return np.array([((lo[w] - hi < r) & (lo - hi[w] < r)).sum() for w in range(T)], np.int32)


def test_tiles_visited():
    frames = [ho.boxes(*inp) for inp in ho.INPUTS] + [ho.boxes(3, 3000, 0.3)]
    for pc in frames:
        res, members, normals, visits = bl.harris_response(dev(pc[None]), want_visits=True)
        want = tiles_expected(pc, 1.0)
        print(pc.shape[1], cpu(visits)[0].tolist())
        assert np.array_equal(cpu(visits)[0], want)
        hr, hm, hn = bl.harris_response_cpu(pc[None], num_threads=16)
        assert np.array_equal(bits(cpu(res)), bits(hr)) and np.array_equal(cpu(members), hm)
    assert (tiles_expected(frames[2], 1.0) < 12).all()                   # (2, 3000, 5): every workgroup prunes
    assert tiles_expected(frames[3], 1.0).sum() > tiles_expected(frames[2], 1.0).sum()       # (3, 3000, 1.5): less to prune
    assert (tiles_expected(frames[4], 1.0) == 12).all()                  # x span below r: nothing to prune
    # a ragged batch: the workgroups without a live query walk nothing
    pc, count = host.ragged_batch()
    visits = cpu(bl.harris_response(dev(pc), dev(count), want_visits=True)[3])
    for b, n in enumerate(count):
        T = (n + 255) // 256
        assert np.array_equal(visits[b, :T], tiles_expected(pc[b, :, :n], 1.0)) and (visits[b, T:] == 0).all()


def test_wrong_permutations_and_arguments():
    """A permutation that does not sort, or leaves [0, n), gives wrong values (slots it never names stay unwritten) -- no
    read or write outside the frame: every entry is clamped into [0, n) before it is used."""
    pc = dev(ho.boxes(1, 1000, 3.0)[None])
    for perm in (torch.arange(1000, dtype=torch.int32, device=DEV).flip(0).unsqueeze(0).contiguous(),
                 torch.full((1, 1000), 1 << 30, dtype=torch.int32, device=DEV),
                 torch.full((1, 1000), -7, dtype=torch.int32, device=DEV)):
        normals, nb = ops.harris_normals(pc, None, perm, 1.0, 3)
        res, members = ops.harris_response(pc, None, perm, normals, 1.0)
        assert normals.shape == (1, 3, 1000) and nb.shape == res.shape == members.shape == (1, 1000)
    torch.cuda.synchronize()
    perm = bl.sort_along_x(pc)
    normals, nb = ops.harris_normals(pc, None, perm, 1.0, 3)              # ... and the right one after them is right
    res, members = ops.harris_response(pc, None, perm, normals, 1.0)
    hr, hm, hn = bl.harris_response_cpu(cpu(pc))
    assert np.array_equal(bits(cpu(res)), bits(hr)) and np.array_equal(cpu(members), hm)
    assert np.array_equal(bits(cpu(normals)), bits(hn))
    with pytest.raises(RuntimeError):
        ops.harris_normals(pc.cpu(), None, perm, 1.0, 3)
    with pytest.raises(RuntimeError):
        ops.harris_normals(pc, None, perm, 0.0, 3)
    with pytest.raises(RuntimeError):
        ops.harris_normals(pc, None, perm, 1.0, 0)
    with pytest.raises(RuntimeError):
        ops.harris_normals(pc, None, perm, float("inf"), 3)               # USIP_EINVAL from the library
    with pytest.raises(RuntimeError):
        ops.harris_response(pc, None, perm, normals.float(), 1.0)
    with pytest.raises(RuntimeError):
        ops.harris_response(pc, None, perm.long(), normals, 1.0)
    with pytest.raises(RuntimeError):
        ops.harris_response(pc, None, perm, normals, 1.0, "moravec")
    with pytest.raises(RuntimeError):
        ops.harris_response(pc, None, perm, normals, float("nan"))
    with pytest.raises(ValueError):
        bl.harris_keypoints(pc, radius=-1.0)
    with pytest.raises(ValueError):
        bl.harris_keypoints(pc, normals=normals)                         # supplied normals are float32


def test_selection_equals_the_twin():
    pc, count = host.ragged_batch()
    det = bl.HarrisDetector(num=16, seed=3)
    kp, cnt = det(dev(pc), dev(count), [5, 6, 7])
    assert len(det.last) == 4
    hm = bl.harris_keypoints_cpu(pc, count, num_threads=16)[0]
    hk, hc = bl.select_keypoints_cpu(pc, hm, count, 16, True, 3, [5, 6, 7])
    assert np.array_equal(cpu(kp), hk) and np.array_equal(cpu(cnt), hc) and hc.tolist() == [16, 16, 1]


def test_no_host_synchronisation_in_harris_keypoints():
    pc, count = host.ragged_batch()
    p, c = dev(pc), dev(count)
    bl.harris_keypoints(p, c)                                            # (the first call loads the code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = bl.harris_keypoints(p, c)                                  # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    h = bl.harris_keypoints_cpu(pc, count, num_threads=16)
    for a, b in zip(out, h):
        assert np.array_equal(bits(cpu(a)), bits(b))


def test_evaluators_take_harris_keypoints():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 2, 4096)      # frame 1 = frame 0 moved by a known pose
    top, seed = 64, 2
    evaluator = ex.build_evaluator("ball", None, top=top, nms_radius=1.0, max_trials=500, seed=seed, method="harris")
    ex.add_scans(evaluator, scans, nodes=128, seed=seed, method="harris")
    twin = {}
    for fid, rows in scans:
        pc = np.ascontiguousarray(rows.T[None, :3])
        m = bl.harris_keypoints_cpu(pc, num_threads=16)[0]
        twin[fid] = bl.select_keypoints_cpu(pc, m, None, top, True, seed, [fid])
        got = evaluator.frames[fid]
        assert np.array_equal(cpu(got[0]), twin[fid][0][0]) and int(got[2]) == int(twin[fid][1][0]) == top
    s = evaluator.evaluate(pairs)
    a, q, gt = pairs[0]
    want = ev.repeatability_cpu(twin[a][0], twin[a][1], twin[q][0], twin[q][1], np.asarray(gt)[None], 0.5)[0]
    assert s["per_pair"]["repeatability"][0] == want[0] and s["keypoint_num_mean"] == top
    # the indoor evaluator likewise
    fe = fr.FragmentEvaluator(None, evaluator.descriptor, evaluator.opt, DEV, top=top)
    fid, rows = scans[0]
    t = dev(rows.T)
    pc, sn = t[:3].unsqueeze(0).contiguous(), t[3:].unsqueeze(0).contiguous()
    kp, count = bl.HarrisDetector(num=top, seed=seed)(pc, None, [fid])
    got = fe.add_fragment_keypoints(fid, pc, sn, kp, count, rows[:, :3])
    assert len(got) == 4 and tuple(got[0].shape) == (3, top) and tuple(got[3].shape) == (4096, 3)
    assert np.array_equal(cpu(got[0]), twin[fid][0][0]) and torch.equal(got[1], evaluator.frames[fid][1])
