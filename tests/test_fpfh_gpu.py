"""The f-19 FPFH kernels on the MI355X (csrc/fpfh.hip) against the library's host twin, which runs the same header
(csrc/fpfh_math.h) over ALL pairs of a frame.  Device and host twin are held to equality as bit patterns: the integer SPFH
counts and member counts, the float64 normals and FPFH, the float32 descriptors, the keypoint member counts -- which is also
what proves the SPFH pass's pruned walk and the gather's pruned range exact and the gather's sums taken in the contract's order.
Inputs: tests/test_fpfh_cpu.py.  No shape is larger than B = 2, N = 1500, M = 300.

tiles_visited: a workgroup walks exactly the tiles of the x-sorted frame that intersect [xlo - r, xhi + r] (counted here in
numpy from the sorted x)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import test_fpfh_cpu as host
from conftest import ROOT
from usip_amd import baselines as bl
from usip_amd import evaluation as ev
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = host.bits
NAMES = ("spfh", "members", "normals", "desc", "kp_members", "fpfh")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return t.cpu().numpy()


def same_as_twin(pc, kp, count=None, kp_count=None, radius=1.0, normal_radius=0.8, normals=None, min_neighbors=3, pc_dev=None):
    """pc [B,3,N], kp [B,3,M] -> the device's (spfh, members, normals, desc, kp_members, fpfh, visited) on the host, after the
    bit-for-bit comparison with the twin"""
    p = dev(pc) if pc_dev is None else pc_dev
    spfh, members, nrm, visited = bl.fpfh_spfh(p, dev(count), radius, dev(normals), normal_radius, min_neighbors,
                                               want_visits=True)
    desc, kpm, fpfh = bl.fpfh_descriptors(p, dev(kp), dev(count), dev(kp_count), radius, dev(normals), normal_radius, True,
                                          min_neighbors)
    d = tuple(cpu(t) for t in (spfh, members, nrm, desc, kpm, fpfh))
    h = bl.fpfh_spfh_cpu(pc, count, radius, normals, normal_radius, min_neighbors, num_threads=16) + \
        bl.fpfh_descriptors_cpu(pc, kp, count, kp_count, radius, normals, normal_radius, True, min_neighbors, num_threads=16)
    for name, a, b in zip(NAMES, d, h):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (name, len(bad), bad[:5].tolist())
    assert np.array_equal(d[3], np.transpose(d[5].astype(np.float32), (0, 2, 1)))       # f32 is the cast of the f64 result
    return d + (cpu(visited),)


def keypoints_around(pc, seed, m, radius):
    """host.keypoints_of plus, from m >= 8 on, keypoints with x below and above the whole cloud: within the radius of its
    ends and beyond it"""
    kp = host.keypoints_of(pc, seed, m)
    if m >= 8:
        lo, hi = pc[0].min(), pc[0].max()
        kp[0, :4] = [lo - 0.5 * radius, hi + 0.5 * radius, lo - 10.0 * radius, hi + 10.0 * radius]
    return kp


def extent(pc):
    return float(np.sqrt(((pc.max(1) - pc.min(1)) ** 2).sum()))


def spacing(pc):
    d = pc.T[:, None, :].astype(np.float64) - pc.T[None, :, :]
    d2 = (d * d).sum(-1) + np.eye(pc.shape[1]) * 1e30
    return float(np.sqrt(d2.min()))


# N -> (count, M): every N at which the tile count or the tail changes, every M at which the wave count of a workgroup does
SHAPES = {1: (None, 1), 2: (None, 63), 255: (None, 64), 256: (None, 65), 257: (None, 300), 600: (513, 65)}


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_small_frames_at_three_radii(n):
    count, m = SHAPES[n]
    pc = host.cloud(20 + n, n)
    live = pc[:, :count] if count else pc
    radii = [1.0] if n < 2 else [2.0 * extent(live) + 1.0, 0.5 * spacing(live), 1.0]
    for radius in radii:
        kp = keypoints_around(live, n, m, radius)
        nrm = host.unit_normals(n, n)[None] if n < 3 else None         # (fewer than three points estimate no normal)
        out = same_as_twin(pc[None], kp[None], host.arr(count), None, radius, 0.8, nrm)
        spfh, members, kpm, visited = out[0][0], out[1][0], out[4][0], out[6][0]
        has = np.isfinite(out[2][0]).all(0) & (out[2][0] != 0).any(0)
        tiles = (live.shape[1] + 255) // 256
        if radius > extent(live):                                      # every tile is walked, everybody is a member
            assert (visited[:tiles] == tiles).all() and (members[has] == has.sum() - 1).all()
            assert m < 8 or (kpm[:2] == (members > 0).sum()).all()      # (the keypoints beyond the ends, within the radius)
        if n >= 2 and radius < spacing(live):                          # no members at all
            assert (members == 0).all() and (spfh == 0).all() and (kpm == 0).all() and (out[5] == 0.0).all()
        if m >= 8:
            assert (kpm[2:4] == 0).all() and (out[5][0, 2:4] == 0.0).all()      # x beyond the cloud by ten radii
        if count:
            assert (spfh[count:] == 0).all() and (members[count:] == 0).all() and (visited[tiles:] == 0).all()


def test_two_frames_with_different_counts_and_keypoint_counts():
    pc = np.stack([host.cloud(31, 600), host.cloud(32, 600)])
    count, kp_count = np.array([513, 257], np.int32), np.array([300, 64], np.int32)
    pc[0, :, 513:] = np.nan                                             # dead slots: nothing may read them into a result
    pc[1, :, 257:] = np.inf
    kp = np.stack([keypoints_around(pc[0, :, :513], 1, 300, 1.0), keypoints_around(pc[1, :, :257], 2, 300, 1.0)])
    out = same_as_twin(pc, kp, count, kp_count)
    assert out[4][0].max() > 8 and out[4][1, :64].max() > 4 and (out[4][1, 64:] == 0).all() and (out[5][1, 64:] == 0.0).all()
    for b, n in enumerate(count):
        T = (n + 255) // 256
        assert np.array_equal(out[6][b, :T], tiles_expected(pc[b, :, :n], 1.0)) and (out[6][b, T:] == 0).all()


def tiles_expected(pc, r):
    xs = np.sort(pc[0].astype(np.float64), kind="stable")
    n = len(xs)
    T = (n + 255) // 256
    lo, hi = xs[np.arange(T) * 256], xs[np.minimum(np.arange(T) * 256 + 255, n - 1)]
    return np.array([((lo[w] - hi < r) & (lo - hi[w] < r)).sum() for w in range(T)], np.int32)


def test_a_frame_stretched_along_x_skips_tiles():
    pc = host.cloud(33, 1500, 1.5, stretch=8.0)                         # x in [-12, 12], six tiles of about 4 each
    kp = keypoints_around(pc, 3, 65, 1.0)
    out = same_as_twin(pc[None], kp[None], radius=1.0, normal_radius=1.0)
    want = tiles_expected(pc, 1.0)
    print(out[6][0].tolist())
    assert np.array_equal(out[6][0], want) and (want <= 3).all() and want.min() == 2
    assert out[1].max() >= 3 and out[4].max() >= 3


def test_duplicated_x_values_straddling_a_tile_edge():
    pc = host.cloud(34, 600)
    order = np.argsort(pc[0], kind="stable")
    pc[0, order[250:262]] = pc[0, order[250]]                           # twelve equal x over the edge at 256
    pc[0, order[506:518]] = pc[0, order[517]]                           # ... and over the edge at 512
    kp = keypoints_around(pc, 4, 65, 1.0)
    kp[0, 4:6] = pc[0, order[250]], pc[0, order[517]]                   # keypoints AT the duplicated x
    kp[:, 6] = pc[:, order[255]]                                        # a keypoint ON a cloud point
    out = same_as_twin(pc[None], kp[None])
    assert out[4][0, 4:7].min() > 0


def test_supplied_against_estimated_normals():
    pc = host.cloud(35, 400)
    kp = keypoints_around(pc, 5, 64, 1.0)
    nrm = host.unit_normals(9, 400)
    nrm[:, 7] = 0.0
    nrm[1, 8] = np.nan
    nrm[2, 9] = np.inf
    est = same_as_twin(pc[None], kp[None])
    sup = same_as_twin(pc[None], kp[None], normals=nrm[None])
    assert (sup[1][0, 7:10] == 0).all() and (sup[0][0, 7:10] == 0).all()              # no normal: no members, no counts
    assert np.array_equal(sup[2][0][:, 10:], nrm.astype(np.float64)[:, 10:])         # used as given
    assert not np.array_equal(est[0], sup[0])


def test_a_non_contiguous_view_of_the_cloud():
    pc = host.cloud(36, 300)
    wide = torch.zeros((1, 3, 600), dtype=torch.float32, device=DEV)
    wide[:, :, ::2] = dev(pc[None])
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    same_as_twin(pc[None], keypoints_around(pc, 6, 33, 1.0)[None], pc_dev=view)


def device_run(points, normals, keypoints, radius, count=None, kp_count=None, num_threads=2):
    """tests/test_fpfh_cpu.py's run() on the device, after the bit-for-bit comparison with it"""
    pc = np.ascontiguousarray(np.array(points, np.float32).T)[None]
    nr = np.ascontiguousarray(np.array(normals, np.float32).T)[None]
    kp = np.ascontiguousarray(np.array(keypoints, np.float32).T)[None]
    spfh, members, _ = bl.fpfh_spfh(dev(pc), dev(host.arr(count)), radius, dev(nr))
    perm = bl.sort_along_x(dev(pc), dev(host.arr(count)))
    fpfh, kpm = ops.fpfh_gather(dev(pc), dev(host.arr(count)), perm, spfh, members, dev(kp), dev(host.arr(kp_count)), radius)
    got = tuple(cpu(t)[0] for t in (spfh, members, fpfh, kpm))
    for a, b in zip(got, host.run(points, normals, keypoints, radius, count, kp_count)):
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
    twin = host.answers(name)[0]                                        # (what the CPU tests held against the oracle)
    for a, b in zip((out[0], out[1], out[2], out[5], out[4]), twin):
        assert np.array_equal(bits(a[0]), bits(b))


def test_wrong_permutations_and_arguments():
    """A permutation that does not sort, or leaves [0, n), gives wrong values -- no read or write outside the frame: every
    entry is clamped into [0, n) before it is used."""
    pc = dev(host.cloud(37, 1000)[None])
    kp = dev(keypoints_around(host.cloud(37, 1000), 7, 65, 1.0)[None])
    normals = bl.harris_normals(pc, None, 0.8)[0]
    for perm in (torch.arange(1000, dtype=torch.int32, device=DEV).flip(0).unsqueeze(0).contiguous(),
                 torch.full((1, 1000), 1 << 30, dtype=torch.int32, device=DEV),
                 torch.full((1, 1000), -7, dtype=torch.int32, device=DEV)):
        spfh, members = ops.fpfh_spfh(pc, None, perm, normals, 1.0)
        spfh.zero_()                                                    # (slots the permutation never names stay unwritten)
        members.zero_()
        fpfh, kpm = ops.fpfh_gather(pc, None, perm, spfh, members, kp, None, 1.0)
        assert fpfh.shape == (1, 65, 33) and kpm.shape == (1, 65)
    torch.cuda.synchronize()
    perm = bl.sort_along_x(pc)
    spfh, members = ops.fpfh_spfh(pc, None, perm, normals, 1.0)          # ... and the right one after them is right
    h = bl.fpfh_spfh_cpu(cpu(pc), None, 1.0, None, 0.8)
    assert np.array_equal(cpu(spfh), h[0]) and np.array_equal(cpu(members), h[1])
    for call in (lambda: ops.fpfh_spfh(pc.cpu(), None, perm, normals, 1.0),
                 lambda: ops.fpfh_spfh(pc, None, perm, normals, 0.0),
                 lambda: ops.fpfh_spfh(pc, None, perm, normals, float("inf")),          # USIP_EINVAL from the library
                 lambda: ops.fpfh_spfh(pc, None, perm, normals.float(), 1.0),
                 lambda: ops.fpfh_spfh(pc, None, perm.long(), normals, 1.0),
                 lambda: ops.fpfh_spfh(pc, None, perm, None, 1.0),
                 lambda: ops.fpfh_gather(pc, None, perm, spfh, members, kp, None, float("nan")),
                 lambda: ops.fpfh_gather(pc, None, perm, spfh[:, :, :32].contiguous(), members, kp, None, 1.0),
                 lambda: ops.fpfh_gather(pc, None, perm, spfh, members, kp[:, :, :0].contiguous(), None, 1.0),
                 lambda: ops.fpfh_gather(pc, None, perm, spfh, None, kp, None, 1.0),
                 lambda: ops.fpfh_gather(pc, None, perm, spfh, members, kp.double(), None, 1.0)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        bl.fpfh_descriptors(pc, kp, radius=-1.0)
    with pytest.raises(ValueError):
        bl.fpfh_descriptors(pc, kp, normals=normals)                     # supplied normals are float32
    with pytest.raises(ValueError):
        bl.fpfh_descriptors(pc, kp[:, :2])


def test_no_host_synchronisation_in_fpfh_descriptors():
    f = host.frame("ragged")
    p, k, c, kc = dev(f["pc"][None]), dev(f["kp"][None]), dev(host.arr(f["count"])), dev(host.arr(f["kp_count"]))
    fpfh = bl.FpfhDescriptor(f["radius"], f["normal_radius"], f["min_neighbors"])
    fpfh(p, k, c, kc)                                                   # (the first call loads the code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        desc = fpfh(p, k, c, kc)                                        # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(desc.shape) == (1, 33, f["kp"].shape[1]) and desc.dtype == torch.float32 and len(fpfh.last) == 2
    assert np.array_equal(cpu(desc)[0].T, host.answers("ragged")[0][3].astype(np.float32))


def test_the_evaluator_takes_fpfh_descriptors():
    """FpfhDescriptor -> RegistrationEvaluator.add_frame_descriptors -> evaluate on two synthetic frames related by a known
    pose: no detector, no descriptor network; D = 33; the matches are match_descriptors_cpu's on the same descriptors."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 2, 4096)      # frame 1 = frame 0 moved by a known pose
    top, seed = 64, 2
    evaluator = ev.RegistrationEvaluator(None, None, None, DEV, top=top, max_trials=500, seed=seed)
    detect, describe = bl.IssDetector(num=top, seed=seed), bl.FpfhDescriptor()
    held = {}
    for fid, rows in scans:
        pc = dev(np.ascontiguousarray(rows.T[None, :3]))
        kp, count = detect(pc, None, [fid])
        desc = describe(pc, kp, None, count)
        got = evaluator.add_frame_descriptors(fid, kp, desc, count)
        assert tuple(got[0].shape) == (3, top) and tuple(got[1].shape) == (33, top) and int(got[2]) == top
        assert torch.equal(got[1], desc[0]) and float(desc.abs().sum()) > 0
        held[fid] = (cpu(desc), cpu(count))
    s = evaluator.evaluate(pairs)
    a, q, _ = pairs[0]
    want = ev.match_descriptors_cpu(held[a][0], held[q][0], held[a][1], held[q][1])
    assert s["pairs"] == 1 and s["keypoint_num_mean"] == top
    assert np.array_equal(s["per_pair"]["match_idx"], want)
    with pytest.raises(ValueError):
        evaluator.add_frame_descriptors(9, kp, desc[:, :, :5], count)
    with pytest.raises(ValueError):
        evaluator.add_frame_descriptors(9, kp[0], desc, count)
    # fewer than top: padded with the first keypoint, as add_frame_keypoints pads
    got = evaluator.add_frame_descriptors(9, kp[:, :, :10], desc[:, :, :10], count)
    assert tuple(got[1].shape) == (33, top) and int(got[2]) == 10 and torch.equal(got[1][:, 10:], desc[0, :, :1].expand(-1, top - 10))


def test_the_example_scores_iss_with_fpfh_without_a_network(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex

    def no_network(*a, **k):
        raise AssertionError("a network was constructed")

    monkeypatch.setattr(ex, "DescriptorLiteOld", no_network)
    monkeypatch.setattr(ex, "build_detector", no_network)
    monkeypatch.setattr(ex.torch, "load", no_network)
    out = str(tmp_path / "desc")
    monkeypatch.setattr(sys, "argv", ["evaluate_registration.py", "--make-synthetic", str(tmp_path / "data"), "--points", "4096",
                                      "--frames", "2", "--top", "64", "--max-trials", "500", "--method", "iss",
                                      "--descriptor-method", "fpfh", "--write-descriptors", out])
    ex.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    s = json.loads(lines[0])
    assert s["pairs"] == 1 and s["method"] == "iss" and s["descriptor_method"] == "fpfh" and s["keypoint_num_mean"] == 64
    assert s["seeded_weights"] is False                                 # nothing seeded, nothing loaded: there are no weights
    for fid in (0, 1):                                                  # rows [x y z d0 .. d32]
        assert os.path.getsize(os.path.join(out, "%06d.bin" % fid)) == 64 * 36 * 4


@pytest.mark.parametrize("name", sorted(host.golden.CASES))
def test_device_equals_the_bits_pinned_before_the_shared_keypoint_walk(name):
    """tests/golden/make_descriptor_walk_golden.py: what the host twin computed before csrc/keypoint_walk.h held the kernels'
    walk, every entry =="""
    host.golden.check("fpfh", name, host.golden.device(name, "fpfh", DEV), "device")
