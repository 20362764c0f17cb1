"""The FPFH baseline descriptor's host twin (csrc/fpfh_cpu.cpp over csrc/fpfh_math.h) against the independent oracle
(tests/fpfh_oracle.py), its degenerate frames with explicit expectations written as literals, and a stand-alone sanitizer
build.  The device is held to this twin bit for bit in tests/test_fpfh_gpu.py, which borrows the inputs.

Bars against the oracle, valid where no decision sits on a threshold (the oracle's margin above 1e-9, asserted FIRST as a
condition on the input; no pair is excluded and no case skipped): SPFH counts, member counts and keypoint member counts EQUAL.

FPFH (derived, u = 2^-53, n = kp_members of the keypoint; every term is non-negative, so relative errors add and never
cancel).  One side, against exact arithmetic:
  d2            float32 differences in float64 (1 rounding each, squared: 2), three squares (1 each), two additions (1 each):
                <= 5 u
  a term        100 / members (1), 1 / d2 (1, on top of d2's 5), the two products (2): <= 9 u; the oracle divides by d2 instead
                of multiplying by the reciprocal, which is one rounding fewer
  a bin's sum   n terms in ANY order: <= (n - 1) u more, (n + 8) u
  a block's sum eleven such bins (10 additions): <= (n + 18) u; 100 / sum: (n + 19) u
  the result    bin * scale: (n + 8) + (n + 19) + 1 = (2 n + 28) u
Two sides: |twin - oracle| <= (4 n + 56) u |oracle| per bin, to first order in u; the factor 1 + 1e-6 covers the higher orders.
A bin that is zero on one side is zero on the other (equal counts).  Measured on the four frames below: at most 7.2 u."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fpfh_oracle as fo
from conftest import GOLDEN, ROOT
from usip_amd import baselines as bl

sys.path.insert(0, GOLDEN)
import make_descriptor_walk_golden as golden  # noqa: E402

U = 2.0 ** -53
MARGIN = 1e-9


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


# ---------------------------------------------------------------------------------------------------- inputs, shared with the GPU tests
def cloud(seed, n, half=2.0, stretch=1.0):
    """pc f32 [3,n]: n cells of a cubic lattice over a box of half-width `half`, one point per cell, jittered by up to 0.3 of
    the spacing (so no two points are closer than 0.4 of it: two points that share ALL their neighbours would get normals equal
    but for rounding, and |a1| against |a2| would be decided by that rounding); x stretched by `stretch`"""
    rng = np.random.RandomState(seed)
    g = int(np.ceil(n ** (1.0 / 3.0)))
    cells = rng.permutation(g * g * g)[:n]
    ijk = np.stack([cells // (g * g), (cells // g) % g, cells % g]).astype(np.float64)
    pc = ((ijk + 0.5 + rng.uniform(-0.3, 0.3, (3, n))) * (2.0 * half / g) - half).astype(np.float32)
    pc[0] *= np.float32(stretch)
    return pc


def unit_normals(seed, n):
    """f32 [3,n]: random directions (unit to float32 rounding; the contract uses them as given)"""
    v = np.random.RandomState(seed).normal(size=(3, n))
    return (v / np.sqrt((v * v).sum(0))).astype(np.float32)


def keypoints_of(pc, seed, m):
    """f32 [3,m]: half of them cloud points moved a little, half anywhere in the cloud's box -- none ON a cloud point"""
    rng = np.random.RandomState(seed)
    lo, hi = pc.min(1, keepdims=True), pc.max(1, keepdims=True)
    anywhere = rng.uniform(-0.3, 1.3, (3, m)) * (hi - lo) + lo          # (some outside the cloud)
    near = pc[:, rng.randint(0, pc.shape[1], m)] + rng.normal(size=(3, m)) * 0.05
    return np.where(np.arange(m) % 2 == 0, near, anywhere).astype(np.float32)


# name -> (cloud seed, N, count, radius, normal radius, min_neighbors, supplied-normals seed or None, M, kp_count)
FRAMES = {
    "estimated": (1, 300, None, 1.0, 0.8, 3, None, 40, None),
    "supplied": (2, 300, None, 0.9, 0.8, 3, 7, 40, None),
    "ragged": (3, 400, 330, 1.1, 0.9, 3, None, 33, 29),
    "sparse": (4, 200, None, 0.8, 0.9, 9, None, 24, None),              # some points have no normal, some keypoints no member
}


def frame(name):
    seed, n, count, radius, normal_radius, min_neighbors, nseed, m, kp_count = FRAMES[name]
    pc = cloud(seed, n)
    return dict(pc=pc, count=count, radius=radius, normal_radius=normal_radius, min_neighbors=min_neighbors,
                kp=keypoints_of(pc, seed + 100, m), normals=None if nseed is None else unit_normals(nseed, n), kp_count=kp_count)


def arr(c):
    return None if c is None else np.array([c], np.int32)


@functools.lru_cache(maxsize=None)
def answers(name, num_threads=3):
    """(the twin's, the oracle's) answers on one frame, computed once per session; nobody writes into them"""
    f = frame(name)
    nrm = None if f["normals"] is None else f["normals"][None]
    spfh, members, normals = bl.fpfh_spfh_cpu(f["pc"][None], arr(f["count"]), f["radius"], nrm, f["normal_radius"],
                                              f["min_neighbors"], num_threads)
    fpfh, kpm = bl.fpfh_gather_cpu(f["pc"][None], arr(f["count"]), spfh, members, f["kp"][None], arr(f["kp_count"]),
                                   f["radius"], num_threads)
    o_spfh, o_members, m1 = fo.spfh(f["pc"], normals[0], f["radius"], f["count"])
    o_fpfh, o_kpm, m2 = fo.fpfh(f["pc"], o_spfh, o_members, f["kp"], f["radius"], f["count"], f["kp_count"])
    return (spfh[0], members[0], normals[0], fpfh[0], kpm[0]), (o_spfh, o_members, o_fpfh, o_kpm, min(m1, m2))


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_host_twin_against_the_oracle(name):
    (spfh, members, normals, fpfh, kpm), (o_spfh, o_members, o_fpfh, o_kpm, margin) = answers(name)
    print("%s: smallest decision margin %.3e; members <= %d, %d points without a normal, kp_members %d .. %d"
          % (name, margin, members.max(), (~fo.has_normal(normals)).sum(), kpm.min(), kpm.max()))
    assert margin > MARGIN                                              # a condition on the input, first
    assert members.max() >= 8 and o_spfh.sum() > 0                      # (the frame does exercise the histograms)
    assert np.array_equal(spfh, o_spfh) and np.array_equal(members, o_members) and np.array_equal(kpm, o_kpm)
    bar = (4.0 * o_kpm[:, None] + 56.0) * U * (1.0 + 1e-6) * np.abs(o_fpfh)
    err = np.abs(fpfh - o_fpfh)
    worst = (err / np.maximum(np.abs(o_fpfh), 1e-300)).max() / U
    print("fpfh: largest relative error %.2f u (bar (4 n + 56) u, n = kp_members)" % worst)
    assert (err <= bar).all()
    assert np.array_equal(fpfh == 0.0, o_fpfh == 0.0)
    sums = fpfh.reshape(-1, 3, 11).sum(-1)
    assert ((np.abs(sums - 100.0) < 1e-10) | (sums == 0.0)).all() and (sums[kpm == 0] == 0.0).all()     # 100 or nothing


def test_the_sparse_frame_has_points_without_a_normal_and_keypoints_without_a_member():
    (spfh, members, normals, fpfh, kpm), _ = answers("sparse")
    none = ~fo.has_normal(normals)
    assert none.any() and (spfh[none] == 0).all() and (members[none] == 0).all()
    assert (kpm == 0).any() and (fpfh[kpm == 0] == 0.0).all()


def test_descriptors_are_the_cast_of_the_float64_result():
    f = frame("ragged")
    desc, kpm, fpfh = bl.fpfh_descriptors_cpu(f["pc"][None], f["kp"][None], arr(f["count"]), arr(f["kp_count"]), f["radius"],
                                              None, f["normal_radius"], True, f["min_neighbors"])
    assert desc.shape == (1, 33, f["kp"].shape[1]) and desc.dtype == np.float32
    assert np.array_equal(desc[0].T, fpfh[0].astype(np.float32))
    assert np.array_equal(bits(fpfh[0]), bits(answers("ragged")[0][3])) and np.array_equal(kpm[0], answers("ragged")[0][4])
    assert (fpfh[0, 29:] == 0.0).all() and (kpm[0, 29:] == 0).all()     # kp_count < M
    spfh, members = answers("ragged")[0][:2]
    assert (spfh[330:] == 0).all() and (members[330:] == 0).all()       # count < N


def test_thread_count_does_not_change_a_bit():
    a, b = answers("ragged", 1)[0], answers("ragged", 5)[0]
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------------- degenerate frames, literal expectations
Z = [0.0, 0.0, 1.0]


def rows(*hot):
    """an SPFH row with a count per named bin: rows((5, 1), (16, 1)) ..."""
    r = np.zeros(33, np.int32)
    for b, c in hot:
        r[b] = c
    return r


def run(points, normals, keypoints, radius, count=None, kp_count=None, num_threads=2):
    """points [n][3], normals [n][3], keypoints [m][3] as lists -> (spfh [n,33], members [n], fpfh [m,33], kp_members [m])"""
    pc = np.ascontiguousarray(np.array(points, np.float32).T)[None]
    nr = np.ascontiguousarray(np.array(normals, np.float32).T)[None]
    kp = np.ascontiguousarray(np.array(keypoints, np.float32).T)[None]
    spfh, members, _ = bl.fpfh_spfh_cpu(pc, arr(count), radius, nr, num_threads=num_threads)
    fpfh, kpm = bl.fpfh_gather_cpu(pc, arr(count), spfh, members, kp, arr(kp_count), radius, num_threads)
    return spfh[0], members[0], fpfh[0], kpm[0]


def hundred(*bins):
    r = np.zeros(33)
    for b in bins:
        r[b] = 100.0
    return r


DEGENERATE = {}


def degenerate(fn):
    DEGENERATE[fn.__name__] = fn
    return fn


@degenerate
def single_point(run):
    spfh, members, fpfh, kpm = run([[1, 2, 3]], [Z], [[1, 2, 3], [1, 2, 3.5]], 2.0)
    assert (spfh == 0).all() and members.tolist() == [0]
    assert (fpfh == 0.0).all() and kpm.tolist() == [0, 0]               # (a point without members adds to no keypoint)


@degenerate
def two_coincident_points(run):
    # each is the other's member; f4 == 0 adds to no bin; both are gathered and add nothing
    spfh, members, fpfh, kpm = run([[1, 2, 3], [1, 2, 3]], [Z, Z], [[1, 2, 3.5], [1, 2, 3]], 2.0)
    assert (spfh == 0).all() and members.tolist() == [1, 1]
    assert (fpfh == 0.0).all() and kpm.tolist() == [2, 0]


@degenerate
def a_point_without_a_normal_among_members(run):
    # p0 - p1 - p2 along x, p1 without a normal: p0 and p2 are each other's only member.  d = (2, 0, 0), both normals z:
    # a1 = a2 = 0, no swap, f3 = 0 -> bin 5; v = (0, -1, 0), w = (1, 0, 0), f2 = 0 -> bin 5; (x, y) = (1, 0) -> angle 0, bin 5
    for none in ([0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]):
        spfh, members, fpfh, kpm = run([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [Z, none, Z], [[0, 0, 0], [1, 0, 0], [9, 9, 9]], 3.0)
        assert members.tolist() == [1, 0, 1]
        assert np.array_equal(spfh, np.stack([rows((5, 1), (16, 1), (27, 1)), rows(), rows((5, 1), (16, 1), (27, 1))]))
        # a keypoint exactly on a cloud point skips that point (d2 == 0): the keypoint on p0 gathers p2 alone, the one on p1
        # gathers p0 and p2 (p1 has no members); a keypoint with no member gets zeros
        assert kpm.tolist() == [1, 2, 0]
        assert np.array_equal(fpfh, np.stack([hundred(5, 16, 27), hundred(5, 16, 27), hundred()]))


@degenerate
def all_normals_parallel_to_the_line(run):
    # points along z with normals z: v = d x n1 = 0 for every pair: members, and no bin
    spfh, members, fpfh, kpm = run([[0, 0, 0], [0, 0, 1], [0, 0, 2]], [Z, Z, Z], [[0, 0.5, 1]], 1.5)
    assert (spfh == 0).all() and members.tolist() == [1, 2, 1]
    assert (fpfh == 0.0).all() and kpm.tolist() == [3]


@degenerate
def lattice_points_with_axis_normals(run):
    # p0 = (0, 0, 0) with normal z, p1 = (0, 1, 0) with normal x: a1 = a2 = 0 EXACTLY (equality: no swap), f3 = 0 -> bin 5;
    # from p0: v = (1, 0, 0), w = (0, 1, 0), f2 = v . n2 = 1 -> 11 clamped to bin 10, (x, y) = (0, 0) EXACTLY -> bin 5; from p1
    # the same three bins (v = (0, 0, 1), w = (0, -1, 0), f2 = 1)
    spfh, members, fpfh, kpm = run([[0, 0, 0], [0, 1, 0]], [Z, [1, 0, 0]], [[0, 0.5, 0]], 1.5)
    assert members.tolist() == [1, 1]
    assert np.array_equal(spfh, np.stack([rows((5, 1), (21, 1), (27, 1))] * 2))
    assert kpm.tolist() == [2] and np.array_equal(fpfh[0], hundred(5, 21, 27))
    # antiparallel normals: (x, y) = (-1, 0), the angle pi, PCL's clamp: bin 10
    spfh, members, _, _ = run([[0, 0, 0], [1, 0, 0]], [Z, [0, 0, -1]], [[0, 0.5, 0]], 1.5)
    assert members.tolist() == [1, 1] and np.array_equal(spfh[0], rows((10, 1), (16, 1), (27, 1)))
    # |a1| < |a2|: the roles swap.  p0 = (0, 0, 0) with normal x, p1 = (0, 0, 1) with normal z, d = (0, 0, 1): a1 = 0, a2 = 1,
    # so n1 = z, n2 = x, d = (0, 0, -1), f3 = -a2 = -1 -> bin 0; v = d x n1 = 0: NO bin after the swap either way
    spfh, members, _, _ = run([[0, 0, 0], [0, 0, 1]], [[1, 0, 0], Z], [[0, 0.5, 0]], 1.5)
    assert members.tolist() == [1, 1] and (spfh == 0).all()
    # the same with p1 = (1, 0, 1), d = (1, 0, 1): a1 = a2 (1 / sqrt 2 each): equality, no swap: n1 = x, n2 = z, f3 = a1 ->
    # 11 (1 + 0.7071) / 2 = 9.39: bin 9; v = d x n1 = (0, 1, 0), w = n1 x v = (0, 0, 1); f2 = v . n2 = 0 -> bin 5; (x, y) = (0, 1):
    # the angle pi / 2 -> 11 * 0.75 = 8.25: bin 8
    spfh, members, _, _ = run([[0, 0, 0], [1, 0, 1]], [[1, 0, 0], Z], [[0, 0.5, 0]], 1.5)
    assert members.tolist() == [1, 1] and np.array_equal(spfh[0], rows((8, 1), (16, 1), (31, 1)))


@degenerate
def a_keypoint_weighs_by_inverse_squared_distance(run):
    # four points on the x axis with normal z, radius 1.5: members 1, 2, 2, 1, every pair's bins (5, 16, 27) as above.  The
    # keypoint (1.5, 0, 0) gathers p1 and p2 alone (|d| = 0.5): each adds (2 * (100 / 2)) * (1 / 0.25) = 400 per histogram
    spfh, members, fpfh, kpm = run([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], [Z] * 4, [[1.5, 0, 0]], 1.5)
    assert members.tolist() == [1, 2, 2, 1] and np.array_equal(spfh[1], rows((5, 2), (16, 2), (27, 2)))
    spfh, members, fpfh, kpm = run([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], [Z] * 4, [[1.5, 0, 0]], 1.0 + 2.0 ** -20)
    assert members.tolist() == [1, 2, 2, 1] and kpm.tolist() == [2] and np.array_equal(fpfh[0], hundred(5, 16, 27))
    # strict membership: at radius exactly 1 nobody has a member
    spfh, members, fpfh, kpm = run([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], [Z] * 4, [[1.5, 0, 0]], 1.0)
    assert members.tolist() == [0, 0, 0, 0] and (spfh == 0).all() and kpm.tolist() == [0] and (fpfh == 0.0).all()


@degenerate
def counts_outside_and_inside_the_frame(run):
    pts, nrm, kps = [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [Z] * 3, [[0.5, 0, 0], [1.5, 0, 0]]
    full = run(pts, nrm, kps, 1.5)
    assert full[1].tolist() == [1, 2, 1] and full[3].tolist() == [2, 2]   # (p0 is AT 1.5 from the second: strict)
    for count in (3, 4, 1000):                                          # > N: clamped
        for x, y in zip(run(pts, nrm, kps, 1.5, count=count), full):
            assert np.array_equal(bits(x), bits(y))
    spfh, members, fpfh, kpm = run(pts, nrm, kps, 1.5, count=2)         # < N: p2 is not there
    assert members.tolist() == [1, 1, 0] and (spfh[2] == 0).all() and kpm.tolist() == [2, 1]
    for count in (0, -5):                                               # 0: nothing anywhere
        spfh, members, fpfh, kpm = run(pts, nrm, kps, 1.5, count=count)
        assert (spfh == 0).all() and (members == 0).all() and (fpfh == 0.0).all() and (kpm == 0).all()
    spfh, members, fpfh, kpm = run(pts, nrm, kps, 1.5, kp_count=1)      # kp_count < M
    assert kpm.tolist() == [2, 0] and np.array_equal(bits(fpfh[0]), bits(full[2][0])) and (fpfh[1] == 0.0).all()
    spfh, members, fpfh, kpm = run(pts, nrm, kps, 1.5, kp_count=0)      # kp_count 0
    assert kpm.tolist() == [0, 0] and (fpfh == 0.0).all() and np.array_equal(spfh, full[0])


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_frames(name):
    DEGENERATE[name](run)


def test_every_sector_of_the_angle_occurs_and_agrees_with_the_inverse_tangent():
    """h1 is decided without an inverse tangent; the oracle's is floor(11 (np.arctan2(y, x) + pi) / (2 pi)).  On the frame with
    supplied random normals every one of the eleven sectors and of the 2 x 11 bins of f2 and f3 is hit, and every count agrees."""
    (spfh, *_), (o_spfh, *_) = answers("supplied")
    assert np.array_equal(spfh, o_spfh) and (spfh.sum(0) > 0).all()


def test_bad_arguments_raise():
    pc = cloud(1, 16)[None]
    kp = pc[:, :, :4].copy()
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(normal_radius=0.0), dict(normal_radius=float("inf")), dict(min_neighbors=0),
               dict(normals=np.zeros((1, 3, 16), np.float64)), dict(normals=np.zeros((1, 3, 15), np.float32))):
        with pytest.raises((RuntimeError, ValueError)):
            bl.fpfh_descriptors_cpu(pc, kp, **kw)
    with pytest.raises(ValueError):
        bl.fpfh_spfh_cpu(pc[0])                                         # not [B,3,N]
    with pytest.raises(ValueError):
        bl.fpfh_spfh_cpu(pc, count=np.array([1, 2], np.int32))
    with pytest.raises(RuntimeError):
        bl.fpfh_spfh_cpu(np.zeros((1, 3, (1 << 20) + 1), np.float32), normals=np.zeros((1, 3, (1 << 20) + 1), np.float32))
    spfh, members, _ = bl.fpfh_spfh_cpu(pc)
    with pytest.raises(RuntimeError):
        bl.fpfh_gather_cpu(pc, None, spfh, members, np.zeros((1, 3, 0), np.float32), None, 1.0)          # M >= 1
    with pytest.raises(RuntimeError):
        bl.fpfh_gather_cpu(pc, None, spfh, members, np.zeros((1, 3, 65536), np.float32), None, 1.0)      # M <= 65535
    with pytest.raises(RuntimeError):
        bl.fpfh_gather_cpu(pc, None, spfh, members, kp, None, float("nan"))
    with pytest.raises(ValueError):
        bl.fpfh_gather_cpu(pc, None, spfh[:, :, :32], members, kp, None, 1.0)
    with pytest.raises(ValueError):
        bl.fpfh_gather_cpu(pc, None, spfh, members, kp[0], None, 1.0)
    with pytest.raises(ValueError):
        bl.FpfhDescriptor(radius=0.0)
    with pytest.raises(ValueError):
        bl.FpfhDescriptor(normal_radius=float("nan"))
    assert bl.FPFH_DEFAULTS == dict(radius=2.0, normal_radius=1.0, min_neighbors=3)


def test_the_library_refuses_null_pointers_and_limits():
    import ctypes

    from usip_amd import _lib
    L = _lib.lib()
    pc, nrm = np.zeros((1, 3, 4), np.float32), np.zeros((1, 3, 4), np.float64)
    spfh, mem = np.zeros((1, 4, 33), np.int32), np.zeros((1, 4), np.int32)
    kp, out, km = np.zeros((1, 3, 2), np.float32), np.zeros((1, 2, 33)), np.zeros((1, 2), np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                        # noqa: E731
    ok = [p(pc), None, p(nrm), 1, 4, 1.0, p(spfh), p(mem), 1]
    assert L.usip_fpfh_spfh_f32_cpu(*ok) == 0
    for i, bad in ((0, None), (2, None), (6, None), (7, None), (3, 0), (3, 65536), (4, 0), (4, (1 << 20) + 1), (5, 0.0),
                   (5, float("inf"))):
        args = list(ok)
        args[i] = bad
        assert L.usip_fpfh_spfh_f32_cpu(*args) < 0, i
    ok = [p(pc), None, p(spfh), p(mem), p(kp), None, 1, 4, 2, 1.0, p(out), p(km), 1]
    assert L.usip_fpfh_gather_f32_cpu(*ok) == 0
    for i, bad in ((0, None), (2, None), (3, None), (4, None), (10, None), (11, None), (6, 0), (7, 0), (8, 0), (8, 65536),
                   (9, -1.0), (9, float("nan"))):
        args = list(ok)
        args[i] = bad
        assert L.usip_fpfh_gather_f32_cpu(*args) < 0, i


# ---------------------------------------------------------------------------------------------------- the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "fpfh_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# a host compiler: g++ or clang++ where there is one, otherwise the clang++ beside hipcc, which every build here needs anyway
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/fpfh_cpu.cpp: random frames, counts in and out of range, ties,
    non-finite coordinates and normals, keypoints outside the cloud.  It links nothing of the package and is never loaded into
    Python."""
    exe = str(tmp_path / "fpfh_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "fpfh_cpu.cpp"), "-o", exe,
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
    golden.check("fpfh", name, golden.host(name, "fpfh", num_threads), "host twin, %d threads" % num_threads)
