"""The f-17 SIFT3D kernels on the MI355X (csrc/sift.hip) against the library's host twin, which runs the same header
(csrc/sift_math.h) over ALL pairs of a frame, and against the independent oracle (tests/sift_oracle.py).  Device and host twin
are held to equality as bit patterns: the octave clouds, fields and counts, the float64 dog, the 25-lists, the mask, the scale
indices and the selected keypoints -- which is also what proves the device's pruned walks exact and its sums taken in the
contract's order.  Inputs and bars: tests/test_sift_cpu.py.  No shape is larger than B = 3, N = 3000.

tiles_visited: a scale-space workgroup walks exactly the tiles of the x-sorted octave cloud that intersect [xlo - r, xhi + r]
(counted here in numpy from the sorted x), r the walk's radius."""
import os
import sys

import numpy as np
import pytest
import torch

import sift_oracle as so
import test_sift_cpu as host
from conftest import ROOT
from usip_amd import baselines as bl
from usip_amd import evaluation as ev
from usip_amd import fragments as fr
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits
FLAT = ("candidates", "mask", "scale", "octave_count")
OCTAVE = ("cloud", "field", "count", "dog", "idx", "mask", "scale_index")


def dev(a):
    return a if a is None or isinstance(a, str) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same(name, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(bits(a) != bits(b))
    assert len(bad) == 0, "%s: %d entries differ, first %s" % (name, len(bad), bad[:5].tolist())


def same_as_twin(pc, count=None, field="z", **par):
    """pc [B,3,N] -> the device's sift_keypoints results on the host (flat results and per-octave tuples), after the bit-for-bit
    comparison with the twin's"""
    d = bl.sift_keypoints(dev(pc), dev(count), field=dev(field), want_octaves=True, **par)
    h = host.twin(pc, count, field=field, num_threads=16, **par)
    d = tuple(cpu(t) for t in d[:4]) + ([tuple(cpu(t) for t in o) for o in d[4]],)
    for name, a, b in zip(FLAT, d, h):
        same(name, a, b)
    assert len(d[4]) == len(h[4])
    for o, (od, oh) in enumerate(zip(d[4], h[4])):
        for name, a, b in zip(OCTAVE, od, oh):
            same("octave %d %s" % (o, name), a, b)
    return d


@pytest.mark.parametrize("name", sorted(host.golden.CASES))
def test_device_equals_the_bits_pinned_before_the_shared_walk(name):
    """tests/golden/make_baseline_walk_golden.py: what the host twin computed before csrc/ascending_walk.h held the kernels'
    body, every entry ==; on the five-tile case at radius 0.5 also the tiles each workgroup walked (the pruning still prunes)"""
    host.golden.check("sift", name, host.golden.sift_device(name, DEV), "device")


def test_ragged_batch_equals_the_host_twin():
    pc, count = host.ragged_batch()
    out = same_as_twin(pc, count, **host.SMALL)
    assert out[3][:, 0].tolist()[2] == 1 and (out[3][:2] >= 25).all() and (out[3][:, 0] <= count).all()
    for b, n in enumerate(count):
        host.against_oracle(out[4], so.sift(pc[b, :, :n], 2, exp_error=host.exp_error(), **host.SMALL), b)


@pytest.mark.parametrize("name", sorted(so.INPUTS))
def test_oracle_inputs_equal_the_host_twin_and_the_oracle(name):
    out = same_as_twin(so.cloud_of(name)[None], **so.INPUTS[name][1])
    want = host.oracle(name)
    host.against_oracle(out[4], want)
    assert tuple(out[3][0]) == so.CLOUDS[name]
    assert tuple(int(o[5].sum()) for o in out[4]) == so.KEYPOINTS[name]


def test_supplied_field_and_the_other_axes():
    pc = so.cloud_of("A")
    out = same_as_twin(pc[None], field=so.reflectance(pc)[None], **so.INPUTS["A"][1])
    host.against_oracle(out[4], host.oracle("A", supplied=True))
    for axis in ("x", "y"):
        same_as_twin(so.cloud_of("C")[None], field=axis, **so.INPUTS["C"][1])


def test_every_scale_count_and_the_reference_parameters():
    """every instantiation of the scale-space and extrema kernels (S = 4 .. 11), the last at the reference's parameters"""
    pc = so.cloud_of("C")[None]
    for k in range(1, 8):
        same_as_twin(pc, **dict(so.INPUTS["C"][1], n_scales_per_octave=k, n_octaves=1))
    par = {k: v for k, v in bl.SIFT_DEFAULTS.items() if k != "field"}
    out = same_as_twin(pc, **par)
    assert out[4][0][3].shape[1] == 10 and out[3][0].tolist() == [390, 155, 45, 23]
    out = same_as_twin(so.cloud_of("C")[None], **dict(so.INPUTS["C"][1], n_octaves=4))
    host.against_oracle(out[4], host.oracle("C", octaves=4))


def test_degenerate_frames():
    for name, (pc, field, par) in host.degenerate_frames().items():
        out = same_as_twin(pc[None], field=field if isinstance(field, str) else field[None], **par)
        host.check_degenerate(name, pc, out)


def test_frames_that_stop_at_different_octaves():
    pc, count, par = host.staggered_batch()
    out = same_as_twin(pc, count, **par)
    depth = [(out[3][b] >= 25).sum() for b in range(3)]
    assert len(set(depth)) == 3
    for b in range(3):
        for o in range(depth[b], 4):
            assert not out[4][o][5][b].any() and (out[4][o][3][b] == 0).all()
    assert out[1].any()


def test_translation_by_whole_leaves():
    pc = host.quantised()
    moved = pc.copy()
    moved[0] += 8.0
    a, b = same_as_twin(pc[None], **so.INPUTS["A"][1]), same_as_twin(moved[None], **so.INPUTS["A"][1])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and a[1].sum() > 0


def tiles_expected(x, r):
    xs = np.sort(x.astype(np.float64), kind="stable")
    n = len(xs)
    T = (n + 255) // 256
    lo, hi = xs[np.arange(T) * 256], xs[np.minimum(np.arange(T) * 256 + 255, n - 1)]
    return np.array([((lo[w] - hi < r) & (lo - hi[w] < r)).sum() for w in range(T)], np.int32)


def test_tiles_visited():
    pruned = 0
    for name, k in (("A", 3), ("B", 3), ("B", 8), ("C", 2)):
        pc = dev(so.cloud_of(name)[None])
        cloud, fld, cnt = bl.sift_octave(pc, "z", None, 0.5)
        dog, visits = bl.sift_scale_space(cloud, fld, cnt, 0.5, k, want_visits=True)
        n = int(cnt[0])
        r = bl.sift_walk_radius(bl.sift_sigma2(0.5, k))
        want = tiles_expected(cpu(cloud)[0, 0, :n], r)
        T = len(want)
        print(name, k, n, "r = %.3f" % r, cpu(visits)[0].tolist())
        assert np.array_equal(cpu(visits)[0, :T], want) and (cpu(visits)[0, T:] == 0).all()
        pruned += int((want < T).sum())
        same("dog", cpu(dog), bl.sift_scale_space_cpu(cpu(cloud), cpu(fld), cpu(cnt), 0.5, k, num_threads=16))
    assert pruned > 0
    # a ragged batch: the workgroups without a live row, and the frames below 25 rows, walk nothing
    pc, count = host.ragged_batch()
    cloud, fld, cnt = bl.sift_octave(dev(pc), "z", dev(count), 0.5)
    visits = cpu(bl.sift_scale_space(cloud, fld, cnt, 0.5, 3, want_visits=True)[1])
    assert (visits[2] == 0).all() and (visits[:2, 0] == 1).all() and (visits[:2, 1] == 0).all()


def test_wrong_permutations_and_arguments():
    """A permutation or a neighbour list that leaves [0, n) gives wrong values -- no read or write outside the frame: every
    entry is clamped into [0, n) before it is used."""
    pc = dev(so.cloud_of("C")[None])
    cloud, fld, cnt = bl.sift_octave(pc, "z", None, 0.5)
    s2 = bl.sift_sigma2(0.5, 2)
    N = cloud.shape[2]
    for perm in (torch.arange(N, dtype=torch.int32, device=DEV).flip(0).unsqueeze(0).contiguous(),
                 torch.full((1, N), 1 << 30, dtype=torch.int32, device=DEV), torch.full((1, N), -7, dtype=torch.int32, device=DEV)):
        dog = ops.sift_dog(cloud, fld, cnt, perm, s2)
        idx = ops.sift_nearest(cloud, cnt, perm)
        assert dog.shape == (1, 4, N) and idx.shape == (1, N, 25)
    mask, sidx = ops.sift_extrema(dog, torch.full((1, N, 25), 1 << 30, dtype=torch.int32, device=DEV), cnt, 0.02)
    # keys that are not sorted, an order that leaves the frame: wrong rows, at most N of them
    keys = ops.sift_voxel_keys(pc, None, 0.5)
    out, ofld, ocnt = ops.sift_voxel_average(pc, None, 2, keys, torch.full((1, N), -3, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert 0 <= int(ocnt[0]) <= N
    perm = bl.sort_along_x(cloud, cnt)                                   # ... and the right ones after them are right
    same("dog", cpu(ops.sift_dog(cloud, fld, cnt, perm, s2)), bl.sift_dog_cpu(cpu(cloud), cpu(fld), cpu(cnt), s2))
    same("idx", cpu(ops.sift_nearest(cloud, cnt, perm)), bl.sift_nearest_cpu(cpu(cloud), cpu(cnt)))
    with pytest.raises(RuntimeError):
        ops.sift_dog(cloud.cpu(), fld, cnt, perm, s2)
    with pytest.raises(RuntimeError):
        ops.sift_dog(cloud, fld.double(), cnt, perm, s2)
    with pytest.raises(RuntimeError):
        ops.sift_dog(cloud, fld, cnt, perm.long(), s2)
    for bad in (s2[:3], s2[::-1].copy(), np.r_[s2[:-1], np.inf], np.r_[0.0, s2[1:]]):
        with pytest.raises(RuntimeError):
            ops.sift_dog(cloud, fld, cnt, perm, bad)                     # USIP_EINVAL from the library (or the wrapper)
    with pytest.raises(RuntimeError):
        ops.sift_extrema(dog, idx, cnt, -0.1)
    with pytest.raises(RuntimeError):
        ops.sift_extrema(dog[:, :2].contiguous(), idx, cnt, 0.1)
    with pytest.raises(RuntimeError):
        ops.sift_voxel_keys(pc, None, 0.0)
    with pytest.raises(RuntimeError):
        ops.sift_voxel_average(pc, None, 3, keys, perm)
    with pytest.raises(ValueError):
        bl.sift_keypoints(pc, min_scale=-1.0)
    with pytest.raises(ValueError):
        bl.sift_keypoints(pc, n_scales_per_octave=9)
    with pytest.raises(ValueError):
        bl.sift_keypoints(pc, field=fld.double())


def test_selection_equals_the_twin():
    pc, count = host.ragged_batch()
    det = bl.SiftDetector(num=16, seed=3, **host.SMALL)
    kp, cnt = det(dev(pc), dev(count), [5, 6, 7])
    assert len(det.last) == 4
    h = bl.sift_keypoints_cpu(pc, count, num_threads=16, **host.SMALL)
    hk, hc = bl.select_candidates_cpu(pc, count, h[0], h[1], 16, True, 3, [5, 6, 7])
    assert np.array_equal(bits(cpu(kp)), bits(hk)) and np.array_equal(cpu(cnt), hc) and hc.tolist() == [16, 16, 1]
    assert h[1][:2].any()
    for ensure in (True, False):
        for mask in (h[1], np.zeros_like(h[1])):
            d = bl.select_candidates(dev(pc), dev(count), dev(h[0]), dev(mask), 9, ensure, 4, [1, 2, 3], want_index=True)
            t = bl.select_candidates_cpu(pc, count, h[0], mask, 9, ensure, 4, [1, 2, 3], want_index=True)
            for a, b in zip(d, t):
                assert np.array_equal(bits(cpu(a)), bits(b))


def test_no_host_synchronisation_in_sift_keypoints_and_the_detector():
    pc, count = host.ragged_batch()
    p, c = dev(pc), dev(count)
    det = bl.SiftDetector(num=16, seed=3, **host.SMALL)
    bl.sift_keypoints(p, c, **host.SMALL)                                # (the first calls load the code objects)
    det(p, c, [5, 6, 7])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = bl.sift_keypoints(p, c, **host.SMALL)                      # raises if anything synchronises
        kp, cnt = det(p, c, [5, 6, 7])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    h = bl.sift_keypoints_cpu(pc, count, num_threads=16, **host.SMALL)
    for name, a, b in zip(FLAT, out, h):
        same(name, cpu(a), b)
    hk, hc = bl.select_candidates_cpu(pc, count, h[0], h[1], 16, True, 3, [5, 6, 7])
    assert np.array_equal(bits(cpu(kp)), bits(hk)) and np.array_equal(cpu(cnt), hc)


def test_evaluators_take_sift_keypoints():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 2, 4096)      # frame 1 = frame 0 moved by a known pose
    top, seed = 64, 2
    par = dict(min_scale=0.5, n_octaves=2, n_scales_per_octave=3, min_contrast=0.01)
    evaluator = ex.build_evaluator("ball", None, top=top, nms_radius=1.0, max_trials=500, seed=seed, method="sift")
    ex.add_scans(evaluator, scans, nodes=128, seed=seed, method="sift", sift=dict(par, field="z"))
    twin = {}
    for fid, rows in scans:
        pc = np.ascontiguousarray(rows.T[None, :3])
        h = bl.sift_keypoints_cpu(pc, num_threads=16, **par)
        twin[fid] = bl.select_candidates_cpu(pc, None, h[0], h[1], top, True, seed, [fid])
        got = evaluator.frames[fid]
        assert np.array_equal(cpu(got[0]), twin[fid][0][0]) and int(got[2]) == int(twin[fid][1][0]) == top
    s = evaluator.evaluate(pairs)
    a, q, gt = pairs[0]
    want = ev.repeatability_cpu(twin[a][0], twin[a][1], twin[q][0], twin[q][1], np.asarray(gt)[None], 0.5)[0]
    assert s["per_pair"]["repeatability"][0] == want[0] and s["keypoint_num_mean"] == top
    # the curvature column as the field, and the indoor evaluator
    ex.add_scans(evaluator, scans[:1], nodes=128, seed=seed, method="sift", sift=dict(par, field="curvature"))
    fe = fr.FragmentEvaluator(None, evaluator.descriptor, evaluator.opt, DEV, top=top)
    fid, rows = scans[0]
    t = dev(rows.T)
    pc, sn = t[:3].unsqueeze(0).contiguous(), t[3:].unsqueeze(0).contiguous()
    kp, count = bl.SiftDetector(num=top, seed=seed, **par)(pc, None, [fid])
    got = fe.add_fragment_keypoints(fid, pc, sn, kp, count, rows[:, :3])
    assert len(got) == 4 and tuple(got[0].shape) == (3, top) and tuple(got[3].shape) == (4096, 3)
    assert np.array_equal(cpu(got[0]), twin[fid][0][0])
