"""The SHOT baseline descriptor's host twin (csrc/shot_cpu.cpp over csrc/shot_math.h) against the independent oracle
(tests/shot_oracle.py), its degenerate frames with explicit expectations written as literals, and a stand-alone sanitizer
build.  The device is held to this twin bit for bit in tests/test_shot_gpu.py, which borrows the inputs.

The tests run in this order on the same seeded frames, each the precondition of the next:
  1 angle()      csrc/shot_math.h's inverse tangent against np.arctan2 on 2 000 001 directions at random lengths, the axes, the
                 diagonals and signed zeros.  Measured here: EPS_A = 4.4408920985006262e-16 (2^-51); asserted: <= 2 EPS_A, since
                 a grid does not visit every argument.
  2 frames       jittered-lattice frames (tests/test_fpfh_cpu.py's, for its reason), keypoints chosen BY THE ORACLE ALONE so that
                 every decision margin is >= 1e-9, every relative eigen-gap >= 1e-3 and no sign vote is tied (asserted first).
                 lrf_members and both sign decisions EQUAL; every axis within the derived bar of eigh's (shot_oracle.frames:
                 the roundings of the seven sums and of either eigen-solver, over the gap).  Measured: at most 0.004 of the bar.
  3 histograms   with the TWIN'S OWN lrf fed to the oracle: kp_members EQUAL; the hard column of every (keypoint, member) pair
                 EQUAL (the twin's is read off a one-point frame per pair: a member's own column holds at least 2 of its 4, a
                 neighbour at most 1/2; the pairs' integer histograms also add up to the frame's, exactly); hist / 2^32 within
                 the derived per-column bar (shot_oracle.histograms: per member touching the column five quanta of 2^-32, 2 EPS_A
                 (4 / pi) + 2 EPS_A (2 / pi), and the float64 roundings of the offsets).  Measured: at most 0.74 of the bar.
  4 conservation every row's sum of hist <= 4 * 2^32 * kp_members, with equality where no member lacks a neighbour.
  5 literals     degenerate frames.
  6 sanitizers   tests/shot_sanitize_main.cpp."""
import functools
import os
import subprocess

import numpy as np
import pytest

import shot_oracle as so
import test_fpfh_cpu as fp
from conftest import ROOT
from usip_amd import baselines as bl

golden = fp.golden

EPS_A = 4.4408920985006262e-16
MARGIN, GAP = 1e-9, 1e-3
ONE = 1 << 32
bits, cloud, unit_normals, arr = fp.bits, fp.cloud, fp.unit_normals, fp.arr
NAMES = ("desc", "kp_members", "shot", "hist", "lrf", "lrf_members")


# ---------------------------------------------------------------------------------------------------- 1: the inverse tangent
def test_angle_against_arctan2():
    n = 2000001
    theta = -np.pi + 2.0 * np.pi * np.arange(n) / (n - 1)
    length = np.exp(np.random.RandomState(0).uniform(-20.0, 20.0, n))
    y, x = length * np.sin(theta), length * np.cos(theta)
    special = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (3, 3), (-7, 7), (0.0, 0.0), (-0.0, 0.0),
               (0.0, -0.0), (-0.0, -0.0), (-0.0, -1.0), (0.0, -1.0), (-0.0, 1.0), (1.0, -0.0), (-1.0, -0.0), (-1.0, 0.0)]
    y = np.concatenate([y, [s[0] for s in special]]).astype(np.float64)
    x = np.concatenate([x, [s[1] for s in special]]).astype(np.float64)
    got = bl.shot_angle_cpu(y, x)
    want = np.arctan2(y + 0.0, x + 0.0)                                 # (a zero of either sign is +0: the contract)
    worst = np.abs(got - want).max()
    print("angle: largest |difference| %.17g = %.2f EPS_A" % (worst, worst / EPS_A))
    assert worst <= 2.0 * EPS_A
    lit = bl.shot_angle_cpu([0.0, -0.0, 0.0, 1.0, -1.0, -0.0], [0.0, -0.0, -1.0, 0.0, 0.0, -1.0])
    assert lit.tolist() == [0.0, 0.0, np.pi, np.pi / 2, -np.pi / 2, np.pi]                # exact, signed zeros as +0


# ---------------------------------------------------------------------------------------------------- inputs, shared with the GPU tests
# name -> (cloud seed, N, count, radius, normal radius, min_neighbors, supplied-normals seed or None, M, kp_count)
FRAMES = {
    "estimated": (1, 300, None, 1.0, 0.8, 3, None, 40, None),
    "supplied": (2, 300, None, 0.9, 0.8, 3, 7, 40, None),
    "ragged": (3, 400, 330, 1.1, 0.9, 3, None, 33, 29),
    "sparse": (4, 200, None, 0.8, 0.9, 9, None, 24, None),              # some points have no normal, some keypoints no frame
}


@functools.lru_cache(maxsize=None)
def frame(name):
    """The keypoints are the first M of 4 M candidates (tests/test_fpfh_cpu.py's keypoints_of) at which the ORACLE has no tied
    sign vote and no relative eigen-gap below 1e-3 (a keypoint without a frame passes)."""
    seed, n, count, radius, normal_radius, min_neighbors, nseed, m, kp_count = FRAMES[name]
    pc = cloud(seed, n)
    cand = fp.keypoints_of(pc[:, :count] if count else pc, seed + 100, 4 * m)
    o = so.frames(pc, cand, radius, count)
    keep = np.where((o["vote"] > 0) & (o["gap"].min(1) >= GAP))[0][:m]
    assert len(keep) == m
    return dict(pc=pc, count=count, radius=radius, normal_radius=normal_radius, min_neighbors=min_neighbors,
                kp=np.ascontiguousarray(cand[:, keep]), normals=None if nseed is None else unit_normals(nseed, n),
                kp_count=kp_count)


@functools.lru_cache(maxsize=None)
def answers(name, num_threads=3):
    """the twin's (desc, kp_members, shot, hist, lrf, lrf_members, normals) on one frame, batch axis kept; nobody writes into
    them"""
    f = frame(name)
    nrm = None if f["normals"] is None else f["normals"][None]
    out = bl.shot_descriptors_cpu(f["pc"][None], f["kp"][None], arr(f["count"]), arr(f["kp_count"]), f["radius"], nrm,
                                  f["normal_radius"], True, f["min_neighbors"], num_threads)
    normals = bl.harris_normals_cpu(f["pc"][None], arr(f["count"]), f["normal_radius"], f["min_neighbors"], num_threads)[0] \
        if nrm is None else nrm.astype(np.float64)
    return out + (normals,)


# ---------------------------------------------------------------------------------------------------- 2: frames
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_against_eigh(name):
    f, (_, _, _, _, lrf, lrf_members, _) = frame(name), answers(name)
    o = so.frames(f["pc"], f["kp"], f["radius"], f["count"], f["kp_count"])
    fr = o["framed"]
    print("%s: margins %s; %d of %d keypoints have a frame, members <= %d" % (name, o["margins"], fr.sum(), len(fr),
                                                                               o["members"].max()))
    assert min(o["margins"].values()) >= MARGIN and o["margins"]["eig"] >= GAP and o["vote"].min() > 0      # the input, first
    assert fr.sum() >= 8
    assert np.array_equal(lrf_members[0], o["members"])
    assert (lrf[0][~fr] == 0.0).all() and np.array_equal((lrf[0] != 0.0).any(1), fr)
    mine, theirs = lrf[0][fr].reshape(-1, 3, 3), o["lrf"][fr].reshape(-1, 3, 3)
    assert ((mine * theirs).sum(-1) > 0.0).all()                        # both sign decisions (and y's with them)
    err = np.abs(mine - theirs).max(-1)
    ratio = (err / o["bar"][fr][:, None]).max()
    print("axes: largest |difference| %.3e, largest ratio to the bar %.4f (bars %.2e .. %.2e)"
          % (err.max(), ratio, o["bar"][fr].min(), o["bar"][fr].max()))
    assert ratio <= 1.0
    assert np.abs((mine * mine).sum(-1) - 1.0).max() < 1e-14            # unit axes, right-handed
    assert np.abs(np.cross(mine[:, 2], mine[:, 0]) - mine[:, 1]).max() < 1e-15


# ---------------------------------------------------------------------------------------------------- 3: histograms
def hard_columns_of_the_twin(f, normals, lrf, hist, kpm):
    """every (keypoint, member) pair as a frame of its own: one point, one keypoint, the keypoint's frame -> i32 [M,352], the
    members per own column; asserts that the pairs' histograms add up to the frame's"""
    n = so._live(f["pc"], f["count"])
    m = so._live(f["kp"], f["kp_count"])
    p, k = f["pc"].astype(np.float64), f["kp"].astype(np.float64)
    d2 = ((p[:, None, :n] - k[:, :m, None]) ** 2).sum(0)
    q, j = np.nonzero((d2 < f["radius"] ** 2) & (d2 > 0) & so.has_normal(normals[:, :n])[None])
    assert np.array_equal(np.bincount(q, minlength=len(kpm)), kpm)
    h1, _, k1 = bl.shot_hist_cpu(f["pc"][:, j].T[:, :, None], None, normals[:, j].T[:, :, None], f["kp"][:, q].T[:, :, None], None,
                                 lrf[q][:, None, :], f["radius"], 4)
    framed = (lrf[q] != 0.0).any(1)
    assert (k1 == 1).all() and (h1[~framed] == 0).all()
    total = np.zeros_like(hist)
    np.add.at(total, q, h1[:, 0])
    assert np.array_equal(total, hist)                                  # integers: exact
    hard = np.zeros(hist.shape, np.int32)
    np.add.at(hard, (q[framed], h1[framed, 0].argmax(1)), 1)
    assert (h1[framed, 0].max(1) >= 2 * ONE).all()
    return hard


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_histograms_against_the_oracle(name):
    f, (desc, kpm, shot, hist, lrf, _, normals) = frame(name), answers(name)
    o = so.histograms(f["pc"], normals[0], f["kp"], lrf[0], f["radius"], EPS_A, f["count"], f["kp_count"])
    print("%s: margins %s; kp_members %d .. %d" % (name, o["margins"], kpm.min(), kpm.max()))
    assert min(o["margins"].values()) >= MARGIN                         # the input, first
    assert np.array_equal(kpm[0], o["kp_members"]) and kpm.max() >= 5     # (the frame does exercise the histograms)
    assert np.array_equal(hard_columns_of_the_twin(f, normals[0], lrf[0], hist[0], kpm[0]), o["hard"])
    got, touched = hist[0] / float(ONE), o["bar"] > 0.0
    err = np.abs(got - o["hist"])
    assert (got[~touched] == 0.0).all() and (o["hist"][~touched] == 0.0).all()
    ratio = (err[touched] / o["bar"][touched]).max()
    print("hist: largest |difference| %.3e, largest ratio to the bar %.3f" % (err.max(), ratio))
    assert ratio <= 1.0
    # the descriptor: unit rows or zero rows, the f32 cast, and close to the oracle's
    norm = np.sqrt((shot[0] ** 2).sum(1))
    some = hist[0].any(1)
    assert np.abs(norm[some] - 1.0).max() < 1e-14 and (shot[0][~some] == 0.0).all()
    assert np.abs(shot[0] - so.descriptor(o["hist"])).max() < 1e-8
    assert np.array_equal(desc[0].T, shot[0].astype(np.float32)) and desc.shape == (1, 352, f["kp"].shape[1])


def test_the_frames_exercise_what_they_should():
    _, kpm, shot, hist, lrf, lm, normals = answers("sparse")
    assert (~so.has_normal(normals[0])).any()
    none = ~(lrf[0] != 0.0).any(1)
    assert none.any() and (hist[0][none] == 0).all() and (shot[0][none] == 0.0).all() and (lm[0][none] < 5).all()
    _, kpm, shot, hist, lrf, lm, _ = answers("ragged")
    assert (lrf[0, 29:] == 0.0).all() and (lm[0, 29:] == 0).all() and (hist[0, 29:] == 0).all() and (kpm[0, 29:] == 0).all()
    used = np.zeros(352, bool)
    for name in FRAMES:
        used |= answers(name)[3][0].any(0)
    az, el, sh, cb = np.unravel_index(np.nonzero(used)[0], (8, 2, 2, 11))
    assert len(set(az)) == 8 and len(set(el)) == 2 and len(set(sh)) == 2 and len(set(cb)) == 11


def test_thread_count_does_not_change_a_bit():
    for x, y in zip(answers("ragged", 1), answers("ragged", 5)):
        assert np.array_equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------------- 4: conservation
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_a_member_adds_at_most_four(name):
    _, kpm, _, hist, _, _, _ = answers(name)
    assert (hist >= 0).all() and (hist.sum(-1) <= 4 * ONE * kpm.astype(np.int64)).all()


def test_a_member_with_all_its_neighbours_adds_exactly_four():
    """r / 4 < dist < 3 r / 4 and within pi / 4 of the frame's equator: the radial and the elevation neighbour exist (the cosine's
    and the azimuth's always do).  The frame is supplied: the identity."""
    rng = np.random.RandomState(5)
    n, r = 150, 2.0
    z, a = rng.uniform(-0.6, 0.6, n), rng.uniform(-np.pi, np.pi, n)      # |z| < sin(pi / 4)
    v = np.stack([np.sqrt(1.0 - z * z) * np.cos(a), np.sqrt(1.0 - z * z) * np.sin(a), z])
    pc = (v * rng.uniform(0.3 * r, 0.7 * r, n)).astype(np.float32)
    nrm = unit_normals(6, n).astype(np.float64)
    lrf = np.eye(3).reshape(1, 1, 9)
    hist, shot, kpm = bl.shot_hist_cpu(pc[None], None, nrm[None], np.zeros((1, 3, 1), np.float32), None, lrf, r)
    o = so.histograms(pc, nrm, np.zeros((3, 1), np.float32), lrf[0], r, EPS_A)
    assert o["full"].all() and kpm[0, 0] == n
    assert int(hist.sum()) == 4 * ONE * n
    far = (pc * np.float32(1.3)).astype(np.float32)                      # ... and with members beyond 3 r / 4: strictly less
    hist, _, kpm = bl.shot_hist_cpu(far[None], None, nrm[None], np.zeros((1, 3, 1), np.float32), None, lrf, r)
    assert 0 < int(hist.sum()) < 4 * ONE * int(kpm[0, 0])


# ---------------------------------------------------------------------------------------------------- 5: literal degenerate frames
Z = [0.0, 0.0, 1.0]
EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def run(points, normals, keypoints, radius, count=None, kp_count=None, lrf=None, num_threads=2):
    """points [n][3], normals [n][3], keypoints [m][3] as lists, lrf [m][9] to supply frames -> (lrf [m,9], lrf_members [m], hist
    [m,352], shot [m,352], kp_members [m]) of the twin"""
    pc = np.ascontiguousarray(np.array(points, np.float32).T)[None]
    nr = np.ascontiguousarray(np.array(normals, np.float32).T)[None].astype(np.float64)
    kp = np.ascontiguousarray(np.array(keypoints, np.float32).T)[None]
    frames, members = bl.shot_frames_cpu(pc, kp, arr(count), arr(kp_count), radius, num_threads)
    used = frames if lrf is None else np.array(lrf, np.float64)[None]
    hist, shot, kpm = bl.shot_hist_cpu(pc, arr(count), nr, kp, arr(kp_count), used, radius, num_threads)
    return frames[0], members[0], hist[0], shot[0], kpm[0]


def col(az, el, sh, cb):
    return ((az * 2 + el) * 2 + sh) * 11 + cb


def row(*hot):
    r = np.zeros(352, np.int64)
    for c, v in hot:
        r[c] = v
    return r


DEGENERATE = {}


def degenerate(fn):
    DEGENERATE[fn.__name__] = fn
    return fn


FIVE = [[1, 0, 0], [-1, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.25]]    # C is diagonal: no rotation, the frame is exact


@degenerate
def single_point(run):
    lrf, lm, hist, shot, kpm = run([[1, 2, 3]], [Z], [[1, 2, 3], [1, 2, 3.5]], 2.0)
    assert lm.tolist() == [1, 1] and (lrf == 0.0).all() and (hist == 0).all() and (shot == 0.0).all()
    assert kpm.tolist() == [0, 1]                                       # (d2 == 0 is no member of the histogram)


@degenerate
def four_members_give_no_frame_and_five_give_one(run):
    lrf, lm, hist, shot, kpm = run(FIVE[:4], [Z] * 4, [[0, 0, 0]], 2.0)
    assert lm.tolist() == [4] and (lrf == 0.0).all() and kpm.tolist() == [4] and (hist == 0).all() and (shot == 0.0).all()
    # sums: s00 = 2, s11 = 0.75, s22 = 0.109375 over W = 6.75: x = e0 (votes 4 : 1), z = e2 (5 : 0), y = z cross x = e1
    lrf, lm, hist, shot, kpm = run(FIVE, [Z] * 5, [[0, 0, 0]], 2.0)
    assert lm.tolist() == [5] and lrf[0].tolist() == EYE and kpm.tolist() == [5]
    assert int(hist.sum()) <= 4 * ONE * 5 and abs(float((shot * shot).sum()) - 1.0) < 1e-15
    # strict membership: at radius exactly 1 the two points at distance 1 are out
    lrf, lm, _, _, _ = run(FIVE, [Z] * 5, [[0, 0, 0]], 1.0)
    assert lm.tolist() == [3] and (lrf == 0.0).all()


@degenerate
def equal_eigenvalues_take_the_first(run):
    # five rows on a line along y, one of them ON the keypoint: only s11 > 0.  x = e1; the smallest are a00 = a22 = 0: z = e0;
    # y = e0 cross e1 = e2.  Votes on x 3 : 2 (the row at d = 0 votes >= 0)
    line = [[0, 1, 0], [0, -1, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0]]
    lrf, lm, _, _, kpm = run(line, [Z] * 5, [[0, 0, 0]], 2.0)
    assert lm.tolist() == [5] and kpm.tolist() == [4] and lrf[0].tolist() == [0, 1, 0, 0, 0, 1, 1, 0, 0]
    # five rows in the plane z = 0 with s00 == s11: x = e0 (the first of the largest), z = e2
    plane = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0]]
    lrf, lm, _, _, _ = run(plane, [Z] * 5, [[0, 0, 0]], 2.0)
    assert lm.tolist() == [5] and lrf[0].tolist() == EYE


@degenerate
def a_tied_vote_keeps_the_axis(run):
    # on the x axis 1, -1, -0.5, -0.25 and one row above: votes on x 2 : 3 -> x = -e0; a11 = 0 is the smallest: z = e1 (all
    # its dots are 0: 5 : 0); y = e1 cross -e0 = e2
    pts = [[1, 0, 0], [-1, 0, 0], [-0.5, 0, 0], [-0.25, 0, 0], [0, 0, 0.25]]
    lrf, lm, _, _, _ = run(pts, [Z] * 5, [[0, 0, 0]], 2.0)
    assert lm.tolist() == [5] and lrf[0].tolist() == [-1, 0, 0, 0, 0, 1, 0, 1, 0]
    # ... and 0.25 with them: 3 : 3, a tie: x = e0 stays; y = e1 cross e0 = -e2
    lrf, lm, _, _, _ = run(pts + [[0.25, 0, 0]], [Z] * 6, [[0, 0, 0]], 2.0)
    assert lm.tolist() == [6] and lrf[0].tolist() == [1, 0, 0, 0, 0, -1, 0, 1, 0]


@degenerate
def a_member_on_every_threshold_at_once(run):
    # frame = identity (supplied), r = 2.  The member (1, 0, 0) with normal e2: dist == r / 2 (inner shell, offset +1/2), z' == 0
    # (lower half, offset -1/2), on the x axis (sector 4, phi = 0, offset -1/2), c == 1 (cb = 10, offset 0)
    _, _, hist, shot, kpm = run([[1, 0, 0]], [Z], [[0, 0, 0]], 2.0, lrf=[EYE])
    half = ONE // 2
    want = row((col(4, 0, 0, 10), 4 * ONE - 3 * half), (col(4, 0, 1, 10), half), (col(4, 1, 0, 10), half),
               (col(3, 0, 0, 10), half))
    assert kpm.tolist() == [1] and np.array_equal(hist[0], want)
    assert np.array_equal(shot[0], want / np.sqrt(float((want.astype(np.float64) ** 2).sum())))
    # c == -1: cb = 0, offset 0
    _, _, hist, _, _ = run([[1, 0, 0]], [[0, 0, -1]], [[0, 0, 0]], 2.0, lrf=[EYE])
    assert np.array_equal(hist[0], row((col(4, 0, 0, 0), 4 * ONE - 3 * half), (col(4, 0, 1, 0), half), (col(4, 1, 0, 0), half),
                                       (col(3, 0, 0, 0), half)))
    # the axes and the diagonals: the sector that BEGINS at the direction; pi belongs to sector 7
    for p, az in (([1, 0, 0], 4), ([1, 1, 0], 5), ([0, 1, 0], 6), ([-1, 1, 0], 7), ([-1, 0, 0], 7), ([-1, -1, 0], 1),
                  ([0, -1, 0], 2), ([1, -1, 0], 3), ([0, 0, 1], 4), ([0, 0, -1], 4)):
        _, _, hist, _, _ = run([p], [Z], [[0, 0, 0]], 4.0, lrf=[EYE])
        own = int(hist[0].argmax())
        assert own // 44 == az and hist[0, own] >= 2 * ONE, (p, own)
        assert (own // 22) % 2 == (1 if p[2] > 0 else 0) and own % 11 == 10
    # straight up and straight down there is no elevation neighbour: the offset's share is dropped
    _, _, hist, _, _ = run([[0, 0, 1]], [Z], [[0, 0, 0]], 4.0, lrf=[EYE])
    assert int(hist.sum()) == 4 * ONE - half                            # (dist = r / 4 is the inner shell's centre: offset 0)
    # ... and nearer than r / 4 there is no neighbour towards the centre either: dist = r / 8, offset -1/4
    _, _, hist, _, _ = run([[0, 0, -0.5]], [Z], [[0, 0, 0]], 4.0, lrf=[EYE])
    assert int(hist.sum()) == 4 * ONE - half - ONE // 4


@degenerate
def a_member_without_a_normal(run):
    for none in ([0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]):
        lrf, lm, hist, _, kpm = run(FIVE, [Z, none, Z, Z, Z], [[0, 0, 0]], 2.0)
        assert lm.tolist() == [5] and lrf[0].tolist() == EYE and kpm.tolist() == [4]     # the frame needs no normal
        full = run(FIVE[:1] + FIVE[2:], [Z] * 4, [[0, 0, 0]], 2.0, lrf=[EYE])
        assert np.array_equal(hist, full[2])


@degenerate
def counts_outside_and_inside_the_frame(run):
    kps = [[0, 0, 0], [0.25, 0, 0]]
    full = run(FIVE, [Z] * 5, kps, 2.0)
    assert full[1].tolist() == [5, 5] and full[4].tolist() == [5, 5]
    for count in (5, 6, 1000):                                          # > N: clamped
        for x, y in zip(run(FIVE, [Z] * 5, kps, 2.0, count=count), full):
            assert np.array_equal(bits(x), bits(y))
    lrf, lm, hist, shot, kpm = run(FIVE, [Z] * 5, kps, 2.0, count=4)    # < N: the fifth is not there
    assert lm.tolist() == [4, 4] and (lrf == 0.0).all() and kpm.tolist() == [4, 4] and (hist == 0).all()
    for count in (0, -5):
        lrf, lm, hist, shot, kpm = run(FIVE, [Z] * 5, kps, 2.0, count=count)
        assert (lm == 0).all() and (lrf == 0.0).all() and (kpm == 0).all() and (hist == 0).all() and (shot == 0.0).all()
    lrf, lm, hist, shot, kpm = run(FIVE, [Z] * 5, kps, 2.0, kp_count=1)
    assert lm.tolist() == [5, 0] and kpm.tolist() == [5, 0] and (lrf[1] == 0.0).all() and (hist[1] == 0).all()
    assert np.array_equal(bits(shot[0]), bits(full[3][0])) and (shot[1] == 0.0).all()
    lrf, lm, hist, shot, kpm = run(FIVE, [Z] * 5, kps, 2.0, kp_count=0)
    assert (lm == 0).all() and (kpm == 0).all() and (hist == 0).all() and (lrf == 0.0).all()


@degenerate
def a_supplied_row_that_is_no_frame(run):
    for bad in ([0.0] * 9, [np.nan] + EYE[1:], EYE[:8] + [np.inf], [0, 0, 0] + EYE[3:]):
        _, _, hist, shot, kpm = run(FIVE, [Z] * 5, [[0, 0, 0]], 2.0, lrf=[bad])
        assert kpm.tolist() == [5] and (hist == 0).all() and (shot == 0.0).all()


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_frames(name):
    DEGENERATE[name](run)


def test_bad_arguments_raise():
    pc = cloud(1, 16)[None]
    kp = pc[:, :, :4].copy()
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(normal_radius=0.0), dict(normal_radius=float("inf")), dict(min_neighbors=0),
               dict(normals=np.zeros((1, 3, 16), np.float64)), dict(normals=np.zeros((1, 3, 15), np.float32))):
        with pytest.raises((RuntimeError, ValueError)):
            bl.shot_descriptors_cpu(pc, kp, **kw)
    with pytest.raises(ValueError):
        bl.shot_frames_cpu(pc[0], kp)                                   # not [B,3,N]
    with pytest.raises(ValueError):
        bl.shot_frames_cpu(pc, kp[0])
    with pytest.raises(ValueError):
        bl.shot_frames_cpu(pc, kp, count=np.array([1, 2], np.int32))
    with pytest.raises(ValueError):
        bl.shot_frames_cpu(pc, kp, kp_count=np.array([1, 2], np.int32))
    with pytest.raises(RuntimeError):
        bl.shot_frames_cpu(pc, np.zeros((1, 3, 0), np.float32))         # M >= 1
    with pytest.raises(RuntimeError):
        bl.shot_frames_cpu(pc, np.zeros((1, 3, 65536), np.float32))     # M <= 65535
    with pytest.raises(RuntimeError):
        bl.shot_frames_cpu(np.zeros((1, 3, (1 << 20) + 1), np.float32), kp)
    lrf, _ = bl.shot_frames_cpu(pc, kp)
    nrm = np.zeros((1, 3, 16))
    with pytest.raises(ValueError):
        bl.shot_hist_cpu(pc, None, nrm[:, :, :15], kp, None, lrf, 1.0)
    with pytest.raises(ValueError):
        bl.shot_hist_cpu(pc, None, nrm, kp, None, lrf[:, :, :8], 1.0)
    with pytest.raises(RuntimeError):
        bl.shot_hist_cpu(pc, None, nrm, kp, None, lrf, float("nan"))
    with pytest.raises(ValueError):
        bl.ShotDescriptor(radius=0.0)
    with pytest.raises(ValueError):
        bl.ShotDescriptor(normal_radius=float("nan"))
    assert bl.SHOT_DEFAULTS == dict(radius=2.0, normal_radius=1.0, min_neighbors=3) and bl.ShotDescriptor.dim == 352


def test_the_library_refuses_null_pointers_and_limits():
    import ctypes

    from usip_amd import _lib
    L = _lib.lib()
    pc, nrm = np.zeros((1, 3, 4), np.float32), np.zeros((1, 3, 4), np.float64)
    kp, lrf, lm = np.zeros((1, 3, 2), np.float32), np.zeros((1, 2, 9)), np.zeros((1, 2), np.int32)
    hist, shot, km = np.zeros((1, 2, 352), np.int64), np.zeros((1, 2, 352)), np.zeros((1, 2), np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                        # noqa: E731
    ok = [p(pc), None, p(kp), None, 1, 4, 2, 1.0, p(lrf), p(lm), 1]
    assert L.usip_shot_lrf_f32_cpu(*ok) == 0
    for i, bad in ((0, None), (2, None), (8, None), (9, None), (4, 0), (4, 65536), (5, 0), (5, (1 << 20) + 1), (6, 0),
                   (6, 65536), (7, 0.0), (7, -1.0), (7, float("inf")), (7, float("nan"))):
        args = list(ok)
        args[i] = bad
        assert L.usip_shot_lrf_f32_cpu(*args) < 0, i
    ok = [p(pc), None, p(nrm), p(kp), None, p(lrf), 1, 4, 2, 1.0, p(hist), p(shot), p(km), 1]
    assert L.usip_shot_hist_f32_cpu(*ok) == 0
    for i, bad in ((0, None), (2, None), (3, None), (5, None), (10, None), (11, None), (12, None), (6, 0), (7, 0), (8, 0),
                   (8, 65536), (9, -1.0), (9, float("nan"))):
        args = list(ok)
        args[i] = bad
        assert L.usip_shot_hist_f32_cpu(*args) < 0, i
    assert L.usip_shot_angle_f64_cpu(None, None, 0, None) < 0


# ---------------------------------------------------------------------------------------------------- 6: the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "shot_sanitize_main.cpp")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/shot_cpu.cpp: random frames, counts in and out of range, ties, non-finite
    coordinates, normals and frames, keypoints outside the cloud.  It links nothing of the package and is never loaded into
    Python."""
    exe = str(tmp_path / "shot_sanitize")
    subprocess.run([fp.CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "shot_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout


# ---------------------------------------------------------------------------------------------------- the bits pinned at one commit
@pytest.mark.parametrize("num_threads", [1, 3])
@pytest.mark.parametrize("name", sorted(golden.CASES))
def test_twin_equals_the_bits_pinned_before_the_shared_keypoint_loop(name, num_threads):
    """tests/golden/make_descriptor_walk_golden.py: what this twin computed before csrc/keypoints_host.h and
    csrc/keypoint_walk.h, every entry =="""
    golden.check("shot", name, golden.host(name, "shot", num_threads), "host twin, %d threads" % num_threads)
