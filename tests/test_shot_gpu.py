"""The f-20 SHOT kernels on the MI355X (csrc/shot.hip) against the library's host twin, which runs the same header
(csrc/shot_math.h) over ALL pairs of a frame.  Device and host twin are held to equality as bit patterns: the float64 frames
and their member counts, the integer histograms, the keypoint member counts, the float64 descriptors and their float32 cast --
which is also what proves the pruned range [lo, hi) exact, the frame's sums taken in the contract's order and the LDS integer
adds complete.  Inputs: tests/test_shot_cpu.py.  No shape is larger than B = 2, N = 600, M = 300."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import test_shot_cpu as host
from conftest import ROOT
from usip_amd import baselines as bl
from usip_amd import evaluation as ev
from usip_amd import inference, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits, ONE = host.bits, host.ONE


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same_as_twin(pc, kp, count=None, kp_count=None, radius=1.0, normal_radius=0.8, normals=None, min_neighbors=3, pc_dev=None):
    """pc [B,3,N], kp [B,3,M] -> the device's (desc, kp_members, shot, hist, lrf, lrf_members) on the host, after the bit-for-bit
    comparison with the twin"""
    p = dev(pc) if pc_dev is None else pc_dev
    d = tuple(cpu(t) for t in bl.shot_descriptors(p, dev(kp), dev(count), dev(kp_count), radius, dev(normals), normal_radius,
                                                   True, min_neighbors))
    h = bl.shot_descriptors_cpu(pc, kp, count, kp_count, radius, normals, normal_radius, True, min_neighbors, num_threads=16)
    for name, a, b in zip(host.NAMES, d, h):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (name, len(bad), bad[:5].tolist())
    assert np.array_equal(d[0], np.transpose(d[2].astype(np.float32), (0, 2, 1)))       # f32 is the cast of the f64 result
    lrf, lm = bl.shot_frames(p, dev(kp), dev(count), dev(kp_count), radius)             # the frames on their own
    assert np.array_equal(bits(cpu(lrf)), bits(d[4])) and np.array_equal(cpu(lm), d[5])
    return d


def keypoints_around(pc, seed, m, radius):
    """tests/test_fpfh_cpu.py's keypoints_of plus, from m >= 8 on, keypoints with x below and above the whole cloud: within the
    radius of its ends and beyond it (an empty [lo, hi)), and one ON a cloud point"""
    kp = host.fp.keypoints_of(pc, seed, m)
    if m >= 8:
        lo, hi = pc[0].min(), pc[0].max()
        kp[0, :4] = [lo - 0.5 * radius, hi + 0.5 * radius, lo - 10.0 * radius, hi + 10.0 * radius]
        kp[:, 4] = pc[:, pc.shape[1] // 2]
    return kp


def extent(pc):
    return float(np.sqrt(((pc.max(1) - pc.min(1)) ** 2).sum()))


def spacing(pc):
    d = pc.T[:, None, :].astype(np.float64) - pc.T[None, :, :]
    d2 = (d * d).sum(-1) + np.eye(pc.shape[1]) * 1e30
    return float(np.sqrt(d2.min()))


# every N at which a wave's walk changes (one row, fewer than, exactly and more than its 64 lanes, several rounds) crossed with
# every M at which the waves of the last workgroup do (1, 3, 4 busy waves, a second workgroup with 1, many workgroups)
COUNTS = {1: None, 2: None, 63: None, 64: None, 65: None, 600: 513}
MS = (1, 3, 4, 5, 300)


@pytest.mark.parametrize("n", sorted(COUNTS))
def test_small_frames_at_three_radii(n):
    count = COUNTS[n]
    pc = host.cloud(20 + n, n)
    live = pc[:, :count] if count else pc
    # beyond the frame's extent (a window of exactly 64 and of 65 rows at N = 64, 65), below its smallest spacing, between
    radii = [1.0] if n < 2 else [2.0 * extent(live) + 1.0, 0.5 * spacing(live), 1.0]
    nrm = host.unit_normals(n, n)[None] if n < 3 else None              # (fewer than three points estimate no normal)
    for m in MS:
        for radius in radii:
            kp = keypoints_around(live, n + m, m, radius)
            desc, kpm, shot, hist, lrf, lm = same_as_twin(pc[None], kp[None], host.arr(count), None, radius, 0.8, nrm)
            if radius > extent(live) and m < 8:                         # everybody is a member of every keypoint's frame
                assert (lm[0] == live.shape[1]).all()
                assert n < 5 or (lrf[0] != 0.0).any(1).all()
            if n >= 2 and 2.0 * radius <= spacing(live):                # at most the point a keypoint sits on
                assert lm.max() <= 1 and (lrf == 0.0).all() and (hist == 0).all() and (shot == 0.0).all()
            if m >= 8:
                assert (lm[0, 2:4] == 0).all() and (kpm[0, 2:4] == 0).all() and (hist[0, 2:4] == 0).all()     # an empty [lo, hi)
                assert lm[0, 4] >= 1                                    # the keypoint ON a cloud point


def test_two_frames_with_different_counts_and_keypoint_counts():
    pc = np.stack([host.cloud(31, 600), host.cloud(32, 600)])
    count, kp_count = np.array([513, 257], np.int32), np.array([300, 64], np.int32)
    pc[0, :, 513:] = np.nan                                             # dead slots: nothing may read them into a result
    pc[1, :, 257:] = np.inf
    kp = np.stack([keypoints_around(pc[0, :, :513], 1, 300, 1.0), keypoints_around(pc[1, :, :257], 2, 300, 1.0)])
    desc, kpm, shot, hist, lrf, lm = same_as_twin(pc, kp, count, kp_count)
    assert lm[0].max() > 8 and lm[1, :64].max() > 4 and (lm[1, 64:] == 0).all() and (kpm[1, 64:] == 0).all()
    assert (lrf[1, 64:] == 0.0).all() and (hist[1, 64:] == 0).all() and (shot[1, 64:] == 0.0).all()
    assert hist[0].any() and hist[1, :64].any()


def test_equal_x_values_at_both_ends_of_the_window():
    pc = host.cloud(34, 600)
    order = np.argsort(pc[0], kind="stable")
    pc[0, order[250:262]] = pc[0, order[250]]                           # twelve equal x ...
    pc[0, order[506:518]] = pc[0, order[517]]                           # ... twice
    a, b = pc[0, order[250]], pc[0, order[517]]
    kp = keypoints_around(pc, 4, 65, 1.0)
    kp[0, 5:11] = [a, b, a + np.float32(1.0), a - np.float32(1.0), b + np.float32(1.0), b - np.float32(1.0)]
    kp[1:, 5:11] = pc[1:, order[[250, 517, 250, 250, 517, 517]]]        # the run sits AT lo (q_x - x == r) and AT hi
    out = same_as_twin(pc[None], kp[None])
    assert out[5][0, 5:7].min() >= 5


def test_more_than_64_members_in_one_column():
    """The contended LDS add.  A wedge of the plane z = 0 seen from the origin under the identity frame: 100 members with normal
    e2, all in sector 4, the lower half, the outer shell and cosine bin 10 -- a wave's 64 lanes add to ONE column at once."""
    rng = np.random.RandomState(8)
    n, r = 100, 2.0
    ang, dist = rng.uniform(np.radians(5), np.radians(40), n), rng.uniform(0.55 * r, 0.95 * r, n)
    pc = np.stack([dist * np.cos(ang), dist * np.sin(ang), np.zeros(n)]).astype(np.float32)
    nrm = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, n))
    kp, lrf = np.zeros((1, 3, 1), np.float32), np.array(host.EYE).reshape(1, 1, 9)
    p = dev(pc[None])
    hist, shot, kpm = (cpu(t) for t in ops.shot_hist(p, None, bl.sort_along_x(p), dev(nrm[None]), dev(kp), None, dev(lrf), r))
    for a, b in zip((hist, shot, kpm), bl.shot_hist_cpu(pc[None], None, nrm[None], kp, None, lrf, r)):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    own = host.col(4, 0, 1, 10)
    assert kpm[0, 0] == n and hist[0, 0, own] >= 2 * ONE * n and hist[0, 0].argmax() == own
    # ... and a lattice plane seen from its centre, frames computed: every member in the lower half and one cosine bin
    g = (np.arange(15) - 7) * 0.1
    plane = np.stack([np.repeat(g, 15), np.tile(g, 15), np.zeros(225)]).astype(np.float32)
    plane[:2] += np.random.RandomState(9).uniform(-0.01, 0.01, (2, 225)).astype(np.float32)
    out = same_as_twin(plane[None], np.zeros((1, 3, 1), np.float32), radius=2.0,
                       normals=np.tile(np.array([[0.0], [0.0], [1.0]], np.float32), (1, 225))[None])
    assert out[5][0, 0] == 225 and out[1][0, 0] == 225 and np.count_nonzero(out[3][0, 0]) <= 2 * 8 * 2 * 2


def test_supplied_against_estimated_normals():
    pc = host.cloud(35, 400)
    kp = keypoints_around(pc, 5, 64, 1.0)
    nrm = host.unit_normals(9, 400)
    nrm[:, 7] = 0.0
    nrm[1, 8] = np.nan
    nrm[2, 9] = np.inf
    est = same_as_twin(pc[None], kp[None])
    sup = same_as_twin(pc[None], kp[None], normals=nrm[None])
    assert np.array_equal(bits(est[4]), bits(sup[4])) and np.array_equal(est[5], sup[5])      # the frames need no normal
    assert not np.array_equal(est[3], sup[3]) and (sup[1] <= est[5]).all()


def test_a_non_contiguous_view_of_the_cloud():
    pc = host.cloud(36, 300)
    wide = torch.zeros((1, 3, 600), dtype=torch.float32, device=DEV)
    wide[:, :, ::2] = dev(pc[None])
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    same_as_twin(pc[None], keypoints_around(pc, 6, 33, 1.0)[None], pc_dev=view)


def device_run(points, normals, keypoints, radius, count=None, kp_count=None, lrf=None, num_threads=2):
    """tests/test_shot_cpu.py's run() on the device, after the bit-for-bit comparison with it"""
    pc = dev(np.ascontiguousarray(np.array(points, np.float32).T)[None])
    nr = dev(np.ascontiguousarray(np.array(normals, np.float32).T)[None].astype(np.float64))
    kp = dev(np.ascontiguousarray(np.array(keypoints, np.float32).T)[None])
    c, kc = dev(host.arr(count)), dev(host.arr(kp_count))
    perm = bl.sort_along_x(pc, c)
    frames, members = ops.shot_lrf(pc, c, perm, kp, kc, radius)
    used = frames if lrf is None else dev(np.array(lrf, np.float64)[None])
    hist, shot, kpm = ops.shot_hist(pc, c, perm, nr, kp, kc, used, radius)
    got = tuple(cpu(t)[0] for t in (frames, members, hist, shot, kpm))
    for a, b in zip(got, host.run(points, normals, keypoints, radius, count, kp_count, lrf)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    return got


@pytest.mark.parametrize("name", sorted(host.DEGENERATE))
def test_degenerate_frames(name):
    host.DEGENERATE[name](device_run)


@pytest.mark.parametrize("name", sorted(host.FRAMES))
def test_the_oracle_frames(name):
    f = host.frame(name)
    out = same_as_twin(f["pc"][None], f["kp"][None], host.arr(f["count"]), host.arr(f["kp_count"]), f["radius"],
                       f["normal_radius"], None if f["normals"] is None else f["normals"][None], f["min_neighbors"])
    for a, b in zip(out, host.answers(name)):                           # (what the CPU tests held against the oracle)
        assert np.array_equal(bits(a), bits(b))


def test_wrong_permutations_and_arguments():
    """A permutation that does not sort, or leaves [0, n), gives wrong values -- no read or write outside the frame: every
    entry is clamped into [0, n) before it is used."""
    pc = dev(host.cloud(37, 1000)[None])
    kp = dev(keypoints_around(host.cloud(37, 1000), 7, 65, 1.0)[None])
    normals = bl.harris_normals(pc, None, 0.8)[0]
    for perm in (torch.arange(1000, dtype=torch.int32, device=DEV).flip(0).unsqueeze(0).contiguous(),
                 torch.full((1, 1000), 1 << 30, dtype=torch.int32, device=DEV),
                 torch.full((1, 1000), -7, dtype=torch.int32, device=DEV)):
        lrf, lm = ops.shot_lrf(pc, None, perm, kp, None, 1.0)
        hist, shot, kpm = ops.shot_hist(pc, None, perm, normals, kp, None, lrf, 1.0)
        assert lrf.shape == (1, 65, 9) and hist.shape == (1, 65, 352) and shot.shape == (1, 65, 352) and kpm.shape == (1, 65)
    torch.cuda.synchronize()
    perm = bl.sort_along_x(pc)
    lrf, lm = ops.shot_lrf(pc, None, perm, kp, None, 1.0)               # ... and the right one after them is right
    h = bl.shot_frames_cpu(cpu(pc), cpu(kp), radius=1.0)
    assert np.array_equal(bits(cpu(lrf)), bits(h[0])) and np.array_equal(cpu(lm), h[1])
    for call in (lambda: ops.shot_lrf(pc.cpu(), None, perm, kp, None, 1.0),
                 lambda: ops.shot_lrf(pc, None, perm, kp, None, 0.0),
                 lambda: ops.shot_lrf(pc, None, perm, kp, None, float("inf")),           # USIP_EINVAL from the library
                 lambda: ops.shot_lrf(pc, None, perm.long(), kp, None, 1.0),
                 lambda: ops.shot_lrf(pc, None, perm, kp.double(), None, 1.0),
                 lambda: ops.shot_lrf(pc, None, perm, kp[:, :, :0].contiguous(), None, 1.0),
                 lambda: ops.shot_hist(pc, None, perm, normals, kp, None, lrf, float("nan")),
                 lambda: ops.shot_hist(pc, None, perm, normals.float(), kp, None, lrf, 1.0),
                 lambda: ops.shot_hist(pc, None, perm, None, kp, None, lrf, 1.0),
                 lambda: ops.shot_hist(pc, None, perm, normals, kp, None, None, 1.0),
                 lambda: ops.shot_hist(pc, None, perm, normals, kp, None, lrf[:, :, :8].contiguous(), 1.0)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        bl.shot_descriptors(pc, kp, radius=-1.0)
    with pytest.raises(ValueError):
        bl.shot_descriptors(pc, kp, normals=normals)                     # supplied normals are float32
    with pytest.raises(ValueError):
        bl.shot_descriptors(pc, kp[:, :2])


def test_no_host_synchronisation_in_shot_descriptors():
    f = host.frame("ragged")
    p, k, c, kc = dev(f["pc"][None]), dev(f["kp"][None]), dev(host.arr(f["count"])), dev(host.arr(f["kp_count"]))
    shot = bl.ShotDescriptor(f["radius"], f["normal_radius"], f["min_neighbors"])
    shot(p, k, c, kc)                                                   # (the first call loads the code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        desc = shot(p, k, c, kc)                                        # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(desc.shape) == (1, 352, f["kp"].shape[1]) and desc.dtype == torch.float32 and len(shot.last) == 2
    assert np.array_equal(cpu(desc), host.answers("ragged")[0])


def test_the_evaluator_takes_shot_descriptors(tmp_path):
    """ShotDescriptor -> RegistrationEvaluator.add_frame_descriptors -> evaluate on two synthetic frames related by a known
    pose: no detector, no descriptor network; D = 352; the matches are match_descriptors_cpu's on the same descriptors; the
    352-column .bin file reads back what was written."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 2, 4096)      # frame 1 = frame 0 moved by a known pose
    top, seed = 64, 2
    evaluator = ev.RegistrationEvaluator(None, None, None, DEV, top=top, max_trials=500, seed=seed)
    detect, describe = bl.IssDetector(num=top, seed=seed), bl.ShotDescriptor()
    held = {}
    for fid, rows in scans:
        pc = dev(np.ascontiguousarray(rows.T[None, :3]))
        kp, count = detect(pc, None, [fid])
        desc = describe(pc, kp, None, count)
        got = evaluator.add_frame_descriptors(fid, kp, desc, count)
        assert tuple(got[0].shape) == (3, top) and tuple(got[1].shape) == (352, top) and int(got[2]) == top
        assert torch.equal(got[1], desc[0]) and float(desc.abs().sum()) > 0
        held[fid] = (cpu(desc), cpu(count))
    s = evaluator.evaluate(pairs)
    a, q, _ = pairs[0]
    want = ev.match_descriptors_cpu(held[a][0], held[q][0], held[a][1], held[q][1])
    assert s["pairs"] == 1 and s["keypoint_num_mean"] == top
    assert np.array_equal(s["per_pair"]["match_idx"], want)
    path = str(tmp_path / "000000.bin")
    xyz, desc = evaluator.frame_arrays(a)
    inference.write_descriptors_bin(path, xyz, desc)
    back = np.fromfile(path, np.float32).reshape(-1, 3 + 352)
    assert np.array_equal(back[:, :3], np.asarray(xyz, np.float32)) and np.array_equal(back[:, 3:], np.asarray(desc, np.float32))
    assert np.array_equal(back[:, 3:], held[a][0][0].T)


def no_network(*a, **k):
    raise AssertionError("a network was constructed or a checkpoint read")


def test_the_example_scores_iss_with_shot_without_a_network(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    monkeypatch.setattr(ex, "DescriptorLiteOld", no_network)
    monkeypatch.setattr(ex, "build_detector", no_network)
    monkeypatch.setattr(ex.torch, "load", no_network)
    out = str(tmp_path / "desc")
    monkeypatch.setattr(sys, "argv", ["evaluate_registration.py", "--make-synthetic", str(tmp_path / "data"), "--points", "4096",
                                      "--frames", "2", "--top", "64", "--max-trials", "500", "--method", "iss",
                                      "--descriptor-method", "shot", "--write-descriptors", out])
    ex.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    s = json.loads(lines[0])
    assert s["pairs"] == 1 and s["method"] == "iss" and s["descriptor_method"] == "shot" and s["keypoint_num_mean"] == 64
    assert s["seeded_weights"] is False                                 # nothing seeded, nothing loaded: there are no weights
    for fid in (0, 1):                                                  # rows [x y z d0 .. d351]
        assert os.path.getsize(os.path.join(out, "%06d.bin" % fid)) == 64 * 355 * 4


def test_the_fragments_example_scores_shot_without_a_network(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_fragments as exf
    monkeypatch.setattr(torch, "load", no_network)
    monkeypatch.setattr(torch.nn.Module, "__init__", no_network)
    out = str(tmp_path / "desc")
    monkeypatch.setattr(sys, "argv", ["evaluate_fragments.py", "--make-synthetic", str(tmp_path / "room"), "--fragments", "3",
                                      "--points", "3000", "--trials", "500", "--descriptor-method", "shot",
                                      "--write-descriptors", out])
    exf.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    s = json.loads(lines[0])
    assert s["descriptor_method"] == "shot" and s["method"] == "results" and s["scenes"]["synthetic"]["pairs"] == 3
    for i in range(3):
        size = os.path.getsize(os.path.join(out, "synthetic", "%d.bin" % i))
        assert size > 0 and size % (355 * 4) == 0


@pytest.mark.parametrize("name", sorted(host.golden.CASES))
def test_device_equals_the_bits_pinned_before_the_shared_keypoint_walk(name):
    """tests/golden/make_descriptor_walk_golden.py: what the host twin computed before csrc/keypoint_walk.h held the kernels'
    walk, every entry =="""
    host.golden.check("shot", name, host.golden.device(name, "shot", DEV), "device")
