"""The f-21 spin-image kernels on the MI355X (csrc/spin.hip) against the library's host twin, which runs the same header
(csrc/spin_math.h) over ALL pairs of a frame.  Device and host twin are held to equality as bit patterns: the integer images,
the keypoint member counts, the float64 descriptors and their float32 cast (and the axes and their member counts, SHOT's) --
which is also what proves the pruned range [lo, hi) exact and the LDS integer adds complete.  Inputs: tests/test_spin_cpu.py.
No shape is larger than B = 2, N = 600, M = 300."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import test_spin_cpu as host
from conftest import ROOT
from usip_amd import baselines as bl
from usip_amd import evaluation as ev
from usip_amd import inference, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits, ONE, WIDTH, STRUCTURES = host.bits, host.ONE, host.WIDTH, host.STRUCTURES


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(t):
    return None if t is None else t.cpu().numpy()


def same_as_twin(pc, kp, count=None, kp_count=None, radius=1.0, structure="rectangular", support=0.0, normals=None,
                 normal_radius=0.8, min_neighbors=3, axes=None, axis_radius=None, pc_dev=None):
    """pc [B,3,N], kp [B,3,M] -> the device's (desc, kp_members, spin, hist, axes, lrf_members) on the host, after the
    bit-for-bit comparison with the twin"""
    p = dev(pc) if pc_dev is None else pc_dev
    d = tuple(cpu(t) for t in bl.spin_descriptors(p, dev(kp), dev(count), dev(kp_count), radius, dev(axes), axis_radius, support,
                                                   dev(normals), normal_radius, True, min_neighbors, structure))
    h = bl.spin_descriptors_cpu(pc, kp, count, kp_count, radius, axes, axis_radius, support, normals, normal_radius, True,
                                min_neighbors, structure, num_threads=16)
    for name, a, b in zip(host.NAMES, d, h):
        if a is None or b is None:
            assert a is None and b is None and name == "lrf_members" and axes is not None
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, name
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, "%s: %d entries differ, first %s" % (name, len(bad), bad[:5].tolist())
    assert np.array_equal(d[0], np.transpose(d[2].astype(np.float32), (0, 2, 1)))       # f32 is the cast of the f64 result
    assert np.array_equal(d[3].sum(-1), ONE * d[1].astype(np.int64))                    # conservation, on the device too
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


def some_axes(seed, m):
    """f64 [1,m,3]: directions of any length; from m >= 8 on rows 5 .. 7 are no axis"""
    a = np.random.RandomState(seed).normal(size=(1, m, 3)) * 3.0
    if m >= 8:
        a[0, 5], a[0, 6, 1], a[0, 7, 2] = 0.0, np.nan, np.inf
    return a


# every N at which a wave's walk changes (one row, fewer than, exactly and more than its 64 lanes, several rounds) crossed with
# every M at which the waves of the last workgroup do (1, 3, 4 busy waves, a second workgroup with 1, many workgroups)
COUNTS = {1: None, 2: None, 63: None, 64: None, 65: None, 600: 513}
MS = (1, 3, 4, 5, 300)


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("n", sorted(COUNTS))
def test_small_frames_at_three_radii(n, structure):
    """Supplied axes: a frame of fewer than five points has no SHOT frame, and the window must be walked all the same."""
    count = COUNTS[n]
    pc = host.cloud(20 + n, n)
    live = pc[:, :count] if count else pc
    # beyond the frame's extent (a window of exactly 64 and of 65 rows at N = 64, 65), below its smallest spacing, between
    radii = [1.0] if n < 2 else [2.0 * extent(live) + 1.0, 0.5 * spacing(live), 1.0]
    for m in MS:
        for radius in radii:
            kp = keypoints_around(live, n + m, m, radius)
            axes = some_axes(n + m, m)
            desc, kpm, spin, hist, _, _ = same_as_twin(pc[None], kp[None], host.arr(count), None, radius, structure, axes=axes)
            if n >= 2 and radius > extent(live) and m < 8 and structure == "radial":        # everybody is a member of everybody
                assert (kpm[0] == live.shape[1]).all()                  # (at n = 1 a keypoint "anywhere in the box" is ON the point)
            if n >= 2 and 2.0 * radius <= spacing(live):                # at most one row in reach, and a keypoint ON it has none
                assert kpm.max() <= 1
            if m >= 8:
                assert (kpm[0, 2:4] == 0).all() and (hist[0, 2:4] == 0).all()               # an empty [lo, hi)
                assert (kpm[0, 5:8] == 0).all() and (hist[0, 5:8] == 0).all() and (spin[0, 5:8] == 0.0).all()      # no axis
            # ... and with the axes of SHOT's frames over the same radius
            same_as_twin(pc[None], kp[None], host.arr(count), None, radius, structure)


@pytest.mark.parametrize("structure", STRUCTURES)
def test_two_frames_with_different_counts_and_keypoint_counts(structure):
    pc = np.stack([host.cloud(31, 600), host.cloud(32, 600)])
    count, kp_count = np.array([513, 257], np.int32), np.array([300, 64], np.int32)
    pc[0, :, 513:] = np.nan                                             # dead slots: nothing may read them into a result
    pc[1, :, 257:] = np.inf
    kp = np.stack([keypoints_around(pc[0, :, :513], 1, 300, 1.0), keypoints_around(pc[1, :, :257], 2, 300, 1.0)])
    desc, kpm, spin, hist, axes, lm = same_as_twin(pc, kp, count, kp_count, structure=structure)
    assert kpm[0].max() > 8 and kpm[1, :64].max() > 4 and (lm[1, 64:] == 0).all() and (kpm[1, 64:] == 0).all()
    assert (axes[1, 64:] == 0.0).all() and (hist[1, 64:] == 0).all() and (spin[1, 64:] == 0.0).all()
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
    for structure in STRUCTURES:
        out = same_as_twin(pc[None], kp[None], structure=structure)
        assert out[5][0, 5:7].min() >= 5 and out[1][0, 5:7].min() >= 4


def test_a_hundred_members_in_one_cell():
    """The contended LDS add: 100 rows in a small box at alpha in (2, 3), beta in (1, 2) of the rectangular structure (bin 1) --
    a wave's 64 lanes add to the same four cells at once."""
    rng = np.random.RandomState(8)
    n = 100
    ang, alpha, beta = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(2.05, 2.95, n), rng.uniform(1.05, 1.95, n)
    pc = np.stack([alpha * np.cos(ang), alpha * np.sin(ang), beta]).astype(np.float32)
    kp, axes = np.zeros((1, 3, 1), np.float32), np.array(host.Z).reshape(1, 1, 3)
    p = dev(pc[None])
    got = tuple(cpu(t) for t in ops.spin_image(p, None, bl.sort_along_x(p), None, dev(kp), None, dev(axes), host.R))
    for a, b in zip(got, bl.spin_image_cpu(pc[None], None, None, kp, None, axes, host.R)):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    hist, spin, kpm = got
    img = hist[0, 0].reshape(9, 17)
    assert kpm[0, 0] == n and int(img[2:4, 9:11].sum()) == n * ONE and np.count_nonzero(img) == 4
    # ... and the radial structure's: dist in (2, 3) of r = 8, elevation within one bin of pi / 16
    th = rng.uniform(np.pi / 16 * 1.1, np.pi / 16 * 1.9, n)
    pc = (np.stack([np.cos(th) * np.cos(ang), np.cos(th) * np.sin(ang), np.sin(th)]) * alpha).astype(np.float32)
    p = dev(pc[None])
    got = tuple(cpu(t) for t in ops.spin_image(p, None, bl.sort_along_x(p), None, dev(kp), None, dev(axes), 8.0, 0.0, "radial"))
    for a, b in zip(got, bl.spin_image_cpu(pc[None], None, None, kp, None, axes, 8.0, 0.0, "radial")):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    assert got[2][0, 0] == n and int(got[0][0, 0].reshape(9, 17)[2:4, 9:11].sum()) == n * ONE


@pytest.mark.parametrize("structure", STRUCTURES)
def test_a_support_angle_with_estimated_and_with_supplied_normals(structure):
    pc = host.cloud(35, 400)
    kp = keypoints_around(pc, 5, 64, 1.0)
    nrm = host.unit_normals(9, 400)
    nrm[:, 7] = 0.0
    nrm[1, 8] = np.nan
    nrm[2, 9] = np.inf
    free = same_as_twin(pc[None], kp[None], structure=structure)
    est = same_as_twin(pc[None], kp[None], structure=structure, support=0.5)
    sup = same_as_twin(pc[None], kp[None], structure=structure, support=0.5, normals=nrm[None])
    assert np.array_equal(bits(est[4]), bits(free[4])) and np.array_equal(bits(sup[4]), bits(free[4]))      # the axes need no normal
    assert (est[1] <= free[1]).all() and (sup[1] <= free[1]).all() and 0 < sup[1].sum() < free[1].sum()
    assert not np.array_equal(est[3], sup[3])
    # without a support angle supplied normals are not read: the same bits as with none
    for a, b in zip(same_as_twin(pc[None], kp[None], structure=structure, normals=nrm[None]), free):
        assert np.array_equal(bits(a), bits(b))


def test_supplied_axes_against_the_frames():
    f = host.frame("estimated")
    pc, kp = f["pc"][None], f["kp"][None]
    for structure in STRUCTURES:
        own = same_as_twin(pc, kp, radius=f["radius"], structure=structure)
        lrf, lm = bl.shot_frames(dev(pc), dev(kp), radius=f["radius"])
        assert np.array_equal(bits(cpu(lrf)[:, :, 6:9]), bits(own[4])) and np.array_equal(cpu(lm), own[5])
        given = same_as_twin(pc, kp, radius=f["radius"], structure=structure, axes=own[4])
        scaled = same_as_twin(pc, kp, radius=f["radius"], structure=structure, axes=own[4] * 4.0)
        for a, b, c in zip(own[:4], given[:4], scaled[:4]):
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))    # (4 v / (4 |v|) is v / |v|, exactly)
        flipped = same_as_twin(pc, kp, radius=f["radius"], structure=structure, axes=-own[4])
        assert not np.array_equal(flipped[3], own[3])
        # a wider axis radius gives other axes, and more keypoints one
        wide = same_as_twin(pc, kp, radius=f["radius"], structure=structure, axis_radius=1.5 * f["radius"])
        assert (wide[5] >= own[5]).all() and not np.array_equal(bits(wide[4]), bits(own[4]))


def test_a_non_contiguous_view_of_the_cloud():
    pc = host.cloud(36, 300)
    wide = torch.zeros((1, 3, 600), dtype=torch.float32, device=DEV)
    wide[:, :, ::2] = dev(pc[None])
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    for structure in STRUCTURES:
        same_as_twin(pc[None], keypoints_around(pc, 6, 33, 1.0)[None], structure=structure, pc_dev=view)


def device_run(points, keypoints, axes, radius=host.R, structure="rectangular", normals=None, support=0.0, count=None,
               kp_count=None, num_threads=2):
    """tests/test_spin_cpu.py's run() on the device, after the bit-for-bit comparison with it"""
    pc = dev(np.ascontiguousarray(np.array(points, np.float32).T)[None])
    kp = dev(np.ascontiguousarray(np.array(keypoints, np.float32).T)[None])
    nr = None if normals is None else dev(np.ascontiguousarray(np.array(normals, np.float64).T)[None])
    c, kc = dev(host.arr(count)), dev(host.arr(kp_count))
    if support == 0.0:
        nr = None                                                       # (the device's entry point takes none then either way)
    out = ops.spin_image(pc, c, bl.sort_along_x(pc, c), nr, kp, kc, dev(np.array(axes, np.float64)[None]), radius, support,
                         structure)
    got = tuple(cpu(t)[0] for t in out)
    for a, b in zip(got, host.run(points, keypoints, axes, radius, structure, normals, support, count, kp_count)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    return got


@pytest.mark.parametrize("name", sorted(host.LITERAL))
def test_literal_cases(name):
    host.LITERAL[name](device_run)


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", sorted(host.FRAMES))
def test_the_oracle_frames(name, structure):
    f = host.frame(name)
    out = same_as_twin(f["pc"][None], f["kp"][None], host.arr(f["count"]), host.arr(f["kp_count"]), f["radius"], structure,
                       f["support"], None if f["supplied"] is None else f["supplied"][None], f["normal_radius"],
                       f["min_neighbors"])
    for a, b in zip(out, host.answers(name, structure)):                # (what the CPU tests held against the oracle)
        assert np.array_equal(bits(a), bits(b))


def test_wrong_permutations_and_arguments():
    """A permutation that does not sort, or leaves [0, n), gives wrong values -- no read or write outside the frame: every
    entry is clamped into [0, n) before it is used."""
    pc = dev(host.cloud(37, 600)[None])
    kp = dev(keypoints_around(host.cloud(37, 600), 7, 65, 1.0)[None])
    normals = bl.harris_normals(pc, None, 0.8)[0]
    good = bl.sort_along_x(pc)
    axes = ops.shot_lrf(pc, None, good, kp, None, 1.0)[0][:, :, 6:9].contiguous()
    for perm in (torch.arange(600, dtype=torch.int32, device=DEV).flip(0).unsqueeze(0).contiguous(),
                 torch.full((1, 600), 1 << 30, dtype=torch.int32, device=DEV),
                 torch.full((1, 600), -7, dtype=torch.int32, device=DEV)):
        for structure in STRUCTURES:
            hist, spin, kpm = ops.spin_image(pc, None, perm, normals, kp, None, axes, 1.0, 0.5, structure)
            assert hist.shape == (1, 65, WIDTH) and spin.shape == (1, 65, WIDTH) and kpm.shape == (1, 65)
    torch.cuda.synchronize()
    hist, spin, kpm = ops.spin_image(pc, None, good, normals, kp, None, axes, 1.0, 0.5)      # ... and the right one after them is right
    h = bl.spin_image_cpu(cpu(pc), None, cpu(normals), cpu(kp), None, cpu(axes), 1.0, 0.5)
    assert np.array_equal(cpu(hist), h[0]) and np.array_equal(bits(cpu(spin)), bits(h[1])) and np.array_equal(cpu(kpm), h[2])
    for call in (lambda: ops.spin_image(pc.cpu(), None, good, None, kp, None, axes, 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, axes, 0.0),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, axes, float("inf")),     # USIP_EINVAL from the library
                 lambda: ops.spin_image(pc, None, None, None, kp, None, axes, 1.0),              # likewise: no permutation
                 lambda: ops.spin_image(pc, None, good.long(), None, kp, None, axes, 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp.double(), None, axes, 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp[:, :, :0].contiguous(), None, axes[:, :0].contiguous(), 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, None, 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, axes.float(), 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, axes[:, :64].contiguous(), 1.0),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, axes, 1.0, 0.5),         # a support angle without normals
                 lambda: ops.spin_image(pc, None, good, normals.float(), kp, None, axes, 1.0, 0.5),
                 lambda: ops.spin_image(pc, None, good, normals, kp, None, axes, 1.0, -0.5),
                 lambda: ops.spin_image(pc, None, good, normals, kp, None, axes, 1.0, 1.5),
                 lambda: ops.spin_image(pc, None, good, normals, kp, None, axes, 1.0, float("nan")),
                 lambda: ops.spin_image(pc, None, good, None, kp, None, axes, 1.0, 0.0, "angular")):
        with pytest.raises(RuntimeError):
            call()
    for kw in (dict(radius=-1.0), dict(axis_radius=0.0), dict(support_angle_cos=2.0), dict(structure="angular"),
               dict(support_angle_cos=0.5, normals=normals),            # supplied normals are float32
               dict(axes=axes.float()), dict(axes=axes[:, :64])):
        with pytest.raises(ValueError):
            bl.spin_descriptors(pc, kp, **kw)
    with pytest.raises(ValueError):
        bl.spin_descriptors(pc, kp[:, :2])


def test_no_host_synchronisation_in_spin_descriptors():
    f = host.frame("supplied")
    p, k = dev(f["pc"][None]), dev(f["kp"][None])
    for structure, support in (("rectangular", 0.0), ("radial", f["support"])):
        spin = bl.SpinDescriptor(f["radius"], None, support, f["normal_radius"], f["min_neighbors"], structure)
        spin(p, k)                                                      # (the first call loads the code objects)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            desc = spin(p, k)                                           # raises if anything synchronises
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert tuple(desc.shape) == (1, WIDTH, f["kp"].shape[1]) and desc.dtype == torch.float32 and len(spin.last) == 2
    supplied = bl.SpinDescriptor(f["radius"], None, f["support"], f["normal_radius"], f["min_neighbors"], "radial")
    assert np.array_equal(cpu(supplied(p, k, None, None, dev(f["supplied"][None]))), host.answers("supplied", "radial")[0])


def test_the_evaluator_takes_spin_descriptors(tmp_path):
    """SpinDescriptor -> RegistrationEvaluator.add_frame_descriptors -> evaluate on two synthetic frames related by a known
    pose: no detector, no descriptor network; D = 153; the matches are match_descriptors_cpu's on the same descriptors; the
    153-column .bin file reads back what was written."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    scans, pairs = ex.make_synthetic(np.random.default_rng(3), 2, 4096)      # frame 1 = frame 0 moved by a known pose
    top, seed = 64, 2
    evaluator = ev.RegistrationEvaluator(None, None, None, DEV, top=top, max_trials=500, seed=seed)
    detect, describe = bl.IssDetector(num=top, seed=seed), bl.SpinDescriptor()
    held = {}
    for fid, rows in scans:
        pc = dev(np.ascontiguousarray(rows.T[None, :3]))
        kp, count = detect(pc, None, [fid])
        desc = describe(pc, kp, None, count)
        got = evaluator.add_frame_descriptors(fid, kp, desc, count)
        assert tuple(got[0].shape) == (3, top) and tuple(got[1].shape) == (WIDTH, top) and int(got[2]) == top
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
    back = np.fromfile(path, np.float32).reshape(-1, 3 + WIDTH)
    assert np.array_equal(back[:, :3], np.asarray(xyz, np.float32)) and np.array_equal(back[:, 3:], np.asarray(desc, np.float32))
    assert np.array_equal(back[:, 3:], held[a][0][0].T)


def no_network(*a, **k):
    raise AssertionError("a network was constructed or a checkpoint read")


def test_the_example_scores_iss_with_spin_without_a_network(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_registration as ex
    monkeypatch.setattr(ex, "DescriptorLiteOld", no_network)
    monkeypatch.setattr(ex, "build_detector", no_network)
    monkeypatch.setattr(ex.torch, "load", no_network)
    out = str(tmp_path / "desc")
    monkeypatch.setattr(sys, "argv", ["evaluate_registration.py", "--make-synthetic", str(tmp_path / "data"), "--points", "4096",
                                      "--frames", "2", "--top", "64", "--max-trials", "500", "--method", "iss",
                                      "--descriptor-method", "spin", "--spin-radius", "2.5", "--spin-axis-radius", "2.0",
                                      "--spin-support-angle-cos", "0.25", "--spin-structure", "radial",
                                      "--write-descriptors", out])
    ex.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    s = json.loads(lines[0])
    assert s["pairs"] == 1 and s["method"] == "iss" and s["descriptor_method"] == "spin" and s["keypoint_num_mean"] == 64
    assert s["seeded_weights"] is False                                 # nothing seeded, nothing loaded: there are no weights
    for fid in (0, 1):                                                  # rows [x y z d0 .. d152]
        assert os.path.getsize(os.path.join(out, "%06d.bin" % fid)) == 64 * 156 * 4


def test_the_fragments_example_scores_spin_without_a_network(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_fragments as exf
    monkeypatch.setattr(torch, "load", no_network)
    monkeypatch.setattr(torch.nn.Module, "__init__", no_network)
    out = str(tmp_path / "desc")
    monkeypatch.setattr(sys, "argv", ["evaluate_fragments.py", "--make-synthetic", str(tmp_path / "room"), "--fragments", "3",
                                      "--points", "3000", "--trials", "500", "--descriptor-method", "spin",
                                      "--write-descriptors", out])
    exf.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    s = json.loads(lines[0])
    assert s["descriptor_method"] == "spin" and s["method"] == "results" and s["scenes"]["synthetic"]["pairs"] == 3
    for i in range(3):
        size = os.path.getsize(os.path.join(out, "synthetic", "%d.bin" % i))
        assert size > 0 and size % (156 * 4) == 0


@pytest.mark.parametrize("name", sorted(host.golden.CASES))
def test_device_equals_the_bits_pinned_before_the_shared_keypoint_walk(name):
    """tests/golden/make_descriptor_walk_golden.py: what the host twin computed before csrc/keypoint_walk.h held the kernels'
    walk, every entry =="""
    host.golden.check("spin", name, host.golden.device(name, "spin", DEV), "device")
