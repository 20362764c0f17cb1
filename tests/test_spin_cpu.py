"""The spin-image baseline descriptor's host twin (csrc/spin_cpu.cpp over csrc/spin_math.h) against the independent oracle
(tests/spin_oracle.py), literal cases with explicit expectations written as integers, and a stand-alone sanitizer build.  The
device is held to this twin bit for bit in tests/test_spin_gpu.py, which borrows the inputs.

  1 cells        jittered-lattice frames (tests/test_fpfh_cpu.py's, for its reason).  The keypoints are the first M of 4 M
                 candidates at which THE ORACLE ALONE reports every decision margin >= 1e-9, in both structures (asserted:
                 the lattice leaves enough of them).  The axes are the twin's own SHOT frames' z rows, fed to the oracle.
                 kp_members and the cell pair (ab, bb) of every (keypoint, member) pair EQUAL the oracle's; the twin's are
                 read off one-point frames, whose integer images also add up to the frame's image, exactly.
  2 images       hist / 2^40 within the derived per-cell bar of the oracle's float image (spin_oracle.image: per member
                 touching the cell two quanta of 2^-20, the float64 roundings of u and v and, in the radial structure, 2 EPS_A
                 over the bin's pi / 16).  Nothing is fitted.  Measured: at most 0.85 of the bar.
  3 conservation every row's sum of hist == 2^40 * kp_members, both structures, with and without a support angle.
  4 literals     members whose four cells are known integers; axes that are none; the support angle; counts; refusals.
  5 sanitizers   tests/spin_sanitize_main.cpp."""
import functools
import os
import subprocess

import numpy as np
import pytest

import spin_oracle as so
import test_fpfh_cpu as fp
from conftest import ROOT
from usip_amd import baselines as bl

golden = fp.golden

EPS_A = 4.4408920985006262e-16                                         # csrc/shot_math.h's inverse tangent against numpy's (8p)
MARGIN = 1e-9
Q, ONE = 1 << 20, 1 << 40
W, COLS, WIDTH = 8, 17, 153
STRUCTURES = ("rectangular", "radial")
bits, cloud, unit_normals, arr = fp.bits, fp.cloud, fp.unit_normals, fp.arr
NAMES = ("desc", "kp_members", "spin", "hist", "axes", "lrf_members")

# name -> (cloud seed, N, count, radius, normal radius, min_neighbors, supplied-normals seed or None, M, kp_count, support)
FRAMES = {
    "estimated": (1, 300, None, 1.0, 0.8, 3, None, 40, None, 0.0),
    "supplied": (2, 300, None, 0.9, 0.8, 3, 7, 40, None, 0.5),
    "ragged": (3, 400, 330, 1.1, 0.9, 3, None, 33, 29, 0.0),
    "sparse": (4, 200, None, 0.8, 0.9, 9, None, 24, None, 0.25),        # some points have no normal, some keypoints no axis
}


@functools.lru_cache(maxsize=None)
def frame(name):
    seed, n, count, radius, normal_radius, min_neighbors, nseed, m, kp_count, support = FRAMES[name]
    pc = cloud(seed, n)
    cand = fp.keypoints_of(pc[:, :count] if count else pc, seed + 200, 4 * m)
    supplied = None if nseed is None else unit_normals(nseed, n)
    normals = None
    if support > 0.0:
        normals = supplied.astype(np.float64) if supplied is not None else \
            bl.harris_normals_cpu(pc[None], arr(count), normal_radius, min_neighbors, 3)[0][0]
    axes = bl.shot_frames_cpu(pc[None], cand[None], arr(count), None, radius, 3)[0][0][:, 6:9]
    margin = np.min([so.image(pc, cand, axes, radius, st, EPS_A, support, normals, count)["margin"] for st in STRUCTURES], 0)
    keep = np.where(margin >= MARGIN)[0][:m]
    assert len(keep) == m, "the lattice leaves %d of %d candidates" % ((margin >= MARGIN).sum(), 4 * m)
    return dict(pc=pc, count=count, radius=radius, normal_radius=normal_radius, min_neighbors=min_neighbors,
                kp=np.ascontiguousarray(cand[:, keep]), supplied=supplied, normals=normals, kp_count=kp_count, support=support)


@functools.lru_cache(maxsize=None)
def answers(name, structure, num_threads=3):
    """the twin's (desc, kp_members, spin, hist, axes, lrf_members) on one frame, batch axis kept; nobody writes into them"""
    f = frame(name)
    nrm = None if f["supplied"] is None else f["supplied"][None]
    return bl.spin_descriptors_cpu(f["pc"][None], f["kp"][None], arr(f["count"]), arr(f["kp_count"]), f["radius"], None, None,
                                   f["support"], nrm, f["normal_radius"], True, f["min_neighbors"], structure, num_threads)


# ---------------------------------------------------------------------------------------------------- 1, 2: against the oracle
def cells_of_the_twin(f, structure, axes, hist, kpm):
    """every (keypoint, row of its sphere) pair as a frame of its own: one point, one keypoint, the keypoint's axis -> i32
    [M,8,16], the members per cell pair; asserts that the pairs' images add up to the frame's"""
    n, m = so._live(f["pc"], f["count"]), so._live(f["kp"], f["kp_count"])
    p, k = f["pc"].astype(np.float64), f["kp"].astype(np.float64)
    d2 = ((p[:, None, :n] - k[:, :m, None]) ** 2).sum(0)
    q, j = np.nonzero((d2 < f["radius"] ** 2) & (d2 > 0))
    nrm = None if f["normals"] is None else f["normals"][:, j].T[:, :, None]
    h1, _, k1 = bl.spin_image_cpu(f["pc"][:, j].T[:, :, None], None, nrm, f["kp"][:, q].T[:, :, None], None, axes[q][:, None, :],
                                  f["radius"], f["support"], structure, 4)
    k1, h1 = k1[:, 0], h1[:, 0]
    assert set(np.unique(k1)) <= {0, 1} and (h1[k1 == 0] == 0).all() and (h1[k1 == 1].sum(1) == ONE).all()
    assert np.array_equal(np.bincount(q, weights=k1, minlength=len(kpm)).astype(np.int32), kpm)
    total = np.zeros_like(hist)
    np.add.at(total, q, h1)
    assert np.array_equal(total, hist)                                  # integers: exact
    img = h1[k1 == 1].reshape(-1, W + 1, COLS) > 0
    ab, bb = img.any(2).argmax(1), img.any(1).argmax(1)                 # the first row and column that hold a weight
    cells = np.zeros((len(kpm), W, 2 * W), np.int32)
    np.add.at(cells, (q[k1 == 1], ab, bb), 1)
    return cells


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_images_against_the_oracle(name, structure):
    f, (desc, kpm, spin, hist, axes, lm) = frame(name), answers(name, structure)
    o = so.image(f["pc"], f["kp"], axes[0], f["radius"], structure, EPS_A, f["support"], f["normals"], f["count"], f["kp_count"])
    print("%s %s: margins %s; kp_members %d .. %d" % (name, structure, o["margins"], kpm.min(), kpm.max()))
    assert min(o["margins"].values()) >= MARGIN                         # the input, first
    assert np.array_equal(kpm[0], o["kp_members"]) and kpm.max() >= 5     # (the frame does exercise the image)
    assert np.array_equal(cells_of_the_twin(f, structure, axes[0], hist[0], kpm[0]), o["cells"])
    got, touched = hist[0] / float(ONE), o["bar"] > 0.0
    err = np.abs(got - o["hist"])
    assert (got[~touched] == 0.0).all() and (o["hist"][~touched] == 0.0).all()
    ratio = (err[touched] / o["bar"][touched]).max()
    print("hist: largest |difference| %.3e, largest ratio to the bar %.3f" % (err.max(), ratio))
    assert ratio <= 1.0
    # the descriptor: rows that sum to 1 or zero rows, the f32 cast, and close to the oracle's
    some = kpm[0] > 0
    assert np.abs(spin[0][some].sum(1) - 1.0).max() < 1e-14 and (spin[0][~some] == 0.0).all()
    assert np.array_equal(spin[0], np.where(some[:, None], hist[0] / (np.maximum(kpm[0], 1)[:, None] * float(ONE)), 0.0))
    assert np.abs(spin[0] - so.descriptor(o["hist"], o["kp_members"])).max() < 1e-5
    assert np.array_equal(desc[0].T, spin[0].astype(np.float32)) and desc.shape == (1, WIDTH, f["kp"].shape[1])


def test_the_frames_exercise_what_they_should():
    f = frame("sparse")
    assert (~so.has_normal(f["normals"])).any()
    for st in STRUCTURES:
        _, kpm, spin, hist, axes, lm = answers("sparse", st)
        none = ~(axes[0] != 0.0).any(1)
        assert none.any() and (hist[0][none] == 0).all() and (spin[0][none] == 0.0).all() and (lm[0][none] < 5).all()
        assert (kpm[0][none] == 0).all()
        _, kpm, spin, hist, axes, lm = answers("ragged", st)
        assert (axes[0, 29:] == 0.0).all() and (lm[0, 29:] == 0).all() and (hist[0, 29:] == 0).all() and (kpm[0, 29:] == 0).all()
    # the cylinder drops rows of the sphere, the support angle drops more; every row and column of the image is used
    assert answers("estimated", "rectangular")[1].sum() < answers("estimated", "radial")[1].sum()
    f = frame("supplied")
    free = bl.spin_descriptors_cpu(f["pc"][None], f["kp"][None], radius=f["radius"], structure="radial")[1]
    assert 0 < answers("supplied", "radial")[1].sum() < free.sum()
    for st in STRUCTURES:
        used = np.zeros(WIDTH, bool)
        for name in FRAMES:
            used |= answers(name, st)[3][0].any(0)
        assert used.reshape(W + 1, COLS).any(1).all() and used.reshape(W + 1, COLS).any(0).all()


def test_thread_count_does_not_change_a_bit():
    for st in STRUCTURES:
        for x, y in zip(answers("ragged", st, 1), answers("ragged", st, 5)):
            assert np.array_equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------------- 3: conservation
@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_a_member_adds_exactly_one(name, structure):
    """FRAMES holds two frames without and two with a support angle"""
    _, kpm, _, hist, _, _ = answers(name, structure)
    assert (hist >= 0).all() and np.array_equal(hist.sum(-1), ONE * kpm.astype(np.int64))


# ---------------------------------------------------------------------------------------------------- 4: literal cases
Z = [0.0, 0.0, 1.0]
R = float.fromhex("0x1.6a09e667f3bccp+3")                               # 8 sqrt 2: the rectangular bin is exactly 1
assert (R * 0.70710678118654757) / 8 == 1.0


def run(points, keypoints, axes, radius=R, structure="rectangular", normals=None, support=0.0, count=None, kp_count=None,
        num_threads=2):
    """points [n][3], keypoints [m][3], axes [m][3], normals [n][3] as lists -> (hist [m,153], spin [m,153], kp_members [m])"""
    pc = np.ascontiguousarray(np.array(points, np.float32).T)[None]
    kp = np.ascontiguousarray(np.array(keypoints, np.float32).T)[None]
    nr = None if normals is None else np.ascontiguousarray(np.array(normals, np.float64).T)[None]
    hist, spin, kpm = bl.spin_image_cpu(pc, arr(count), nr, kp, arr(kp_count), np.array(axes, np.float64)[None], radius, support,
                                        structure, num_threads)
    return hist[0], spin[0], kpm[0]


def row(*hot):
    """((alpha row, beta column), weight) ... -> i64 [153]"""
    r = np.zeros(WIDTH, np.int64)
    for (a, b), v in hot:
        r[a * COLS + b] = v
    return r


LITERAL = {}


def literal(fn):
    LITERAL[fn.__name__] = fn
    return fn


O = [[0, 0, 0]]


@literal
def a_member_on_the_axis_and_one_beside_it(run):
    # beta = bin / 2 on the axis: u = 0, v = 1/2 -> cells (0, 8) and (0, 9), half each; the two cells of row 1 get nothing
    hist, spin, kpm = run([[0, 0, 0.5]], O, [Z])
    want = row(((0, 8), Q * (Q // 2)), ((1, 8), 0), ((0, 9), Q * (Q // 2)), ((1, 9), 0))
    assert kpm.tolist() == [1] and np.array_equal(hist[0], want) and np.array_equal(spin[0], want / float(ONE))
    # alpha = bin / 2 perpendicular to the axis: u = 1/2, v = 0 -> cells (0, 8) and (1, 8)
    hist, _, kpm = run([[0.5, 0, 0]], O, [Z])
    assert kpm.tolist() == [1] and np.array_equal(hist[0], row(((0, 8), (Q // 2) * Q), ((1, 8), (Q // 2) * Q), ((0, 9), 0),
                                                               ((1, 9), 0)))
    # alpha = 1/4, beta = 3/4: weights 3/16, 1/16, 9/16, 3/16 of 2^40
    hist, _, _ = run([[0.25, 0, 0.75]], O, [Z])
    assert np.array_equal(hist[0], row(((0, 8), 3 << 36), ((1, 8), 1 << 36), ((0, 9), 9 << 36), ((1, 9), 3 << 36)))
    # ... and below the keypoint: beta = -3/4 -> floor = -1, column 7, offset 1/4
    hist, _, _ = run([[0, 0.25, -0.75]], O, [Z])
    assert np.array_equal(hist[0], row(((0, 7), 9 << 36), ((1, 7), 3 << 36), ((0, 8), 3 << 36), ((1, 8), 1 << 36)))
    # both together: the descriptor is the mean image
    hist, spin, kpm = run([[0.25, 0, 0.75], [0, 0.25, -0.75]], O, [Z])
    assert kpm.tolist() == [2] and int(hist.sum()) == 2 * ONE and spin[0, 8] == (6 << 36) / float(2 * ONE)


@literal
def a_member_on_a_cell_corner(run):
    hist, _, kpm = run([[1, 0, 2]], O, [Z])                             # u = 1, v = 2 exactly
    assert kpm.tolist() == [1] and np.array_equal(hist[0], row(((1, 10), ONE)))


@literal
def the_cylinder_inside_the_sphere(run):
    # R = 8 sqrt 2: the sphere reaches 11.3, the cylinder is alpha < 8, -8 < beta < 8
    for p, cells in (([0, 0, 7.5], ((0, 15), (0, 16))), ([0, 0, -7.5], ((0, 0), (0, 1))), ([7.5, 0, 0], ((7, 8), (8, 8)))):
        hist, _, kpm = run([p], O, [Z])
        assert kpm.tolist() == [1] and np.array_equal(hist[0], row((cells[0], ONE // 2), (cells[1], ONE // 2))), p
    for p in ([0, 0, 8], [0, 0, -8], [8, 0, 0], [0, 8.5, 0], [3, 0, 9]):
        hist, spin, kpm = run([p], O, [Z])                              # inside the sphere, not in the cylinder
        assert kpm.tolist() == [0] and (hist == 0).all() and (spin == 0.0).all(), p
        assert run([p], O, [Z], structure="radial")[2].tolist() == [1]  # the radial structure keeps the whole sphere
    assert run([[0, 0, 11.5]], O, [Z], structure="radial")[2].tolist() == [0]       # ... and nothing beyond (strict)


@literal
def straight_up_the_axis_in_the_radial_structure(run):
    # r = 8: bin = 1; dist = 2: u = 2; c = 1: theta = pi / 2, v = 8 -> the border rule: column 15 with 2^20 - 1 quanta
    hist, _, kpm = run([[0, 0, 2]], O, [Z], 8.0, "radial")
    assert kpm.tolist() == [1] and np.array_equal(hist[0], row(((2, 15), Q), ((2, 16), Q * (Q - 1))))
    # straight down: v = -8 is column 0, offset 0
    hist, _, _ = run([[0, 0, -2]], O, [Z], 8.0, "radial")
    assert np.array_equal(hist[0], row(((2, 0), ONE)))
    # on the equator: v = 0; dist = 2.5: rows 2 and 3
    hist, _, _ = run([[2.5, 0, 0]], O, [Z], 8.0, "radial")
    assert np.array_equal(hist[0], row(((2, 8), ONE // 2), ((3, 8), ONE // 2)))


@literal
def a_keypoint_on_a_cloud_point(run):
    hist, _, kpm = run([[1, 2, 3], [1, 2, 3.5]], [[1, 2, 3]], [Z])
    assert kpm.tolist() == [1] and np.array_equal(hist[0], row(((0, 8), ONE // 2), ((0, 9), ONE // 2)))
    hist, spin, kpm = run([[1, 2, 3]], [[1, 2, 3]], [Z])
    assert kpm.tolist() == [0] and (hist == 0).all() and (spin == 0.0).all()


MEMBERS = [[0.25, 0, 0.75], [1.5, 0.0, -2.25], [0, 3.0, 4.5], [-2.0, 0, 0.125], [0, -0.5, -6.75]]     # dyadic, off the cell edges


@literal
def a_flipped_axis_mirrors_the_columns(run):
    for st, r in (("rectangular", R), ("radial", 8.0)):
        up, _, ku = run(MEMBERS, O, [Z], r, st)
        down, _, kd = run(MEMBERS, O, [[0, 0, -1]], r, st)
        assert ku.tolist() == kd.tolist() == [5]
        if st == "rectangular":                                         # dyadic offsets: q and 2^20 - q, exactly
            assert np.array_equal(up[0].reshape(W + 1, COLS)[:, ::-1], down[0].reshape(W + 1, COLS))
        else:                                                           # (1 - f truncates one quantum apart from 2^20 - q)
            assert np.abs(up[0].reshape(W + 1, COLS)[:, ::-1] - down[0].reshape(W + 1, COLS)).max() <= 5 * Q


@literal
def supplied_axes_need_no_unit_length(run):
    for st, r in (("rectangular", R), ("radial", 8.0)):
        for v, a in (([0, 0, 3], Z), ([0, 0, 0.125], Z), ([6, 0, 8], [3, 0, 4]), ([0.375, 0, 0.5], [3, 0, 4])):
            for x, y in zip(run(MEMBERS, O, [v], r, st), run(MEMBERS, O, [a], r, st)):
                assert np.array_equal(bits(x), bits(y))


@literal
def rows_that_are_no_axis(run):
    for bad in ([0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [0, 0, -np.inf], [1e200, 0, 0], [1e-200, 0, 0]):
        for st in STRUCTURES:
            hist, spin, kpm = run(MEMBERS, O + O, [bad, Z], 8.0, st)
            assert kpm[0] == 0 and (hist[0] == 0).all() and (spin[0] == 0.0).all() and kpm[1] >= 4, bad


@literal
def the_support_angle(run):
    pts = [[0.25, 0, 0.75], [0.25, 0, 0.75 + 1], [0.25, 0, 0.75 + 2], [0.25, 0, 0.75 + 3]]
    lean = [float(np.sin(np.deg2rad(89.0))), 0.0, float(np.cos(np.deg2rad(89.0)))]
    nrm = [Z, [0, 0, 0], [0, 0, -1], lean]                              # with, without, counter-directed, at 89 degrees
    hist, _, kpm = run(pts, O, [Z], normals=nrm, support=0.5)
    assert kpm.tolist() == [2]
    assert np.array_equal(hist[0], run([pts[0], pts[2]], O, [Z])[0][0])
    assert run(pts, O, [Z], normals=nrm, support=0.0)[2].tolist() == [4]          # no angle: no normal is read
    assert run(pts, O, [Z], normals=None, support=0.0)[2].tolist() == [4]
    assert run(pts, O, [Z], normals=nrm, support=0.01)[2].tolist() == [3]         # cos 89 = 0.01745 passes now
    assert run(pts, O, [Z], normals=nrm, support=1.0)[2].tolist() == [2]          # |n . a| == s is not below s
    for none in ([np.nan, 0, 1], [0, np.inf, 0]):
        assert run(pts, O, [Z], normals=[Z, none, Z, Z], support=0.5)[2].tolist() == [3]
    # normals are used as given: twice as long passes a threshold its direction alone would not
    assert run(pts[:1], O, [Z], normals=[[0, 0.9, 0.4]], support=0.5)[2].tolist() == [0]
    assert run(pts[:1], O, [Z], normals=[[0, 1.8, 0.8]], support=0.5)[2].tolist() == [1]


@literal
def counts_outside_and_inside_the_frame(run):
    kps = [[0, 0, 0], [0.25, 0, 0]]
    full = run(MEMBERS, kps, [Z, Z])
    assert full[2].tolist() == [5, 5]
    for count in (5, 6, 1000):                                          # > N: clamped
        for x, y in zip(run(MEMBERS, kps, [Z, Z], count=count), full):
            assert np.array_equal(bits(x), bits(y))
    hist, _, kpm = run(MEMBERS, kps, [Z, Z], count=4)                   # < N: the fifth is not there
    assert kpm.tolist() == [4, 4] and np.array_equal(hist, run(MEMBERS[:4], kps, [Z, Z])[0])
    for count in (0, -5):
        hist, spin, kpm = run(MEMBERS, kps, [Z, Z], count=count)
        assert (kpm == 0).all() and (hist == 0).all() and (spin == 0.0).all()
    hist, spin, kpm = run(MEMBERS, kps, [Z, Z], kp_count=1)
    assert kpm.tolist() == [5, 0] and (hist[1] == 0).all() and (spin[1] == 0.0).all()
    assert np.array_equal(bits(spin[0]), bits(full[1][0]))
    hist, spin, kpm = run(MEMBERS, kps, [Z, Z], kp_count=0)
    assert (kpm == 0).all() and (hist == 0).all() and (spin == 0.0).all()


@pytest.mark.parametrize("name", sorted(LITERAL))
def test_literal_cases(name):
    LITERAL[name](run)


def test_bad_arguments_raise():
    pc = cloud(1, 16)[None]
    kp = pc[:, :, :4].copy()
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(axis_radius=0.0), dict(axis_radius=float("inf")), dict(support_angle_cos=-0.1),
               dict(support_angle_cos=1.5), dict(support_angle_cos=float("nan")), dict(support_angle_cos=float("inf")),
               dict(normal_radius=0.0), dict(min_neighbors=0), dict(structure="angular"), dict(structure=None),
               dict(support_angle_cos=0.5, normals=np.zeros((1, 3, 16), np.float64)),
               dict(support_angle_cos=0.5, normals=np.zeros((1, 3, 15), np.float32)),
               dict(axes=np.zeros((1, 3, 3)))):
        with pytest.raises((RuntimeError, ValueError)):
            bl.spin_descriptors_cpu(pc, kp, **kw)
    axes = np.zeros((1, 4, 3))
    with pytest.raises(ValueError):
        bl.spin_image_cpu(pc[0], None, None, kp, None, axes, 1.0)       # not [B,3,N]
    with pytest.raises(ValueError):
        bl.spin_image_cpu(pc, None, None, kp[0], None, axes, 1.0)
    with pytest.raises(ValueError):
        bl.spin_image_cpu(pc, np.array([1, 2], np.int32), None, kp, None, axes, 1.0)
    with pytest.raises(ValueError):
        bl.spin_image_cpu(pc, None, np.zeros((1, 3, 15)), kp, None, axes, 1.0, 0.5)
    with pytest.raises(ValueError):
        bl.spin_image_cpu(pc, None, None, kp, None, axes, 1.0, 0.0, "angular")
    with pytest.raises(RuntimeError):
        bl.spin_image_cpu(pc, None, None, kp, None, axes, 1.0, 0.5)     # a support angle without normals
    with pytest.raises(RuntimeError):
        bl.spin_image_cpu(pc, None, None, np.zeros((1, 3, 0), np.float32), None, np.zeros((1, 0, 3)), 1.0)       # M >= 1
    for kw in (dict(radius=0.0), dict(axis_radius=-1.0), dict(support_angle_cos=2.0), dict(structure="angular"),
               dict(normal_radius=float("nan"))):
        with pytest.raises(ValueError):
            bl.SpinDescriptor(**kw)
    assert bl.SPIN_DEFAULTS == dict(radius=2.0, axis_radius=None, support_angle_cos=0.0, normal_radius=1.0, min_neighbors=3,
                                    structure="rectangular") and bl.SpinDescriptor.dim == WIDTH
    assert bl.SpinDescriptor().params == bl.SPIN_DEFAULTS
    import usip_amd
    assert usip_amd.SpinDescriptor is bl.SpinDescriptor


def test_the_library_refuses_null_pointers_and_limits():
    import ctypes

    from usip_amd import _lib
    L = _lib.lib()
    pc, nrm = np.zeros((1, 3, 4), np.float32), np.zeros((1, 3, 4), np.float64)
    kp, axes = np.zeros((1, 3, 2), np.float32), np.zeros((1, 2, 3))
    hist, spin, km = np.zeros((1, 2, WIDTH), np.int64), np.zeros((1, 2, WIDTH)), np.zeros((1, 2), np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                        # noqa: E731
    ok = [p(pc), None, None, p(kp), None, p(axes), 1, 4, 2, 1.0, 0.0, 0, p(hist), p(spin), p(km), 1]
    assert L.usip_spin_image_f32_cpu(*ok) == 0
    for i, bad in ((0, None), (3, None), (5, None), (12, None), (13, None), (14, None), (6, 0), (6, 65536), (7, 0),
                   (7, (1 << 20) + 1), (8, 0), (8, 65536), (9, 0.0), (9, -1.0), (9, float("inf")), (9, float("nan")),
                   (10, -0.5), (10, 1.0000001), (10, float("nan")), (10, float("inf")), (10, 0.5), (11, 2), (11, -1)):
        args = list(ok)
        args[i] = bad
        assert L.usip_spin_image_f32_cpu(*args) < 0, i
    args = list(ok)
    args[2], args[10], args[11] = p(nrm), 1.0, 1                        # the limits themselves are inside
    assert L.usip_spin_image_f32_cpu(*args) == 0


# ---------------------------------------------------------------------------------------------------- 5: the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "spin_sanitize_main.cpp")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/spin_cpu.cpp: random frames, counts in and out of range, ties, non-finite
    coordinates, normals and axes, keypoints outside the cloud.  It links nothing of the package and is never loaded into
    Python."""
    exe = str(tmp_path / "spin_sanitize")
    subprocess.run([fp.CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "spin_cpu.cpp"), "-o", exe,
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
    golden.check("spin", name, golden.host(name, "spin", num_threads), "host twin, %d threads" % num_threads)
