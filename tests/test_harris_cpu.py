"""The Harris3D baseline detector's host twin (csrc/harris_cpu.cpp over csrc/harris_math.h) against the independent oracle
(tests/harris_oracle.py), its degenerate frames with explicit expectations, and a stand-alone sanitizer build.  The device is
held to this twin bit for bit in tests/test_harris_gpu.py, which borrows the inputs.

Bars against the oracle, valid where no decision sits on a threshold (the oracle's three margins above 1e-9, asserted first
as a condition on the input): the keypoint index set, `neighbours` and `members` identical.

Supplied normals: |response - oracle| <= 1e-12 -- C's entries are bounded by 1 (by 1.2 for the noisy normals used here), its
sums have at most 713 terms each rounded within 1.1e-16, and no eigenvector is in the path.

Estimated normals (DESIGN 8k has the derivation): either side's covariance entries carry at most 3 (m + 8) u T0 of rounding
(u = 1.1e-16, m members, T0 = sum |d|^2: m-term sums of products, and the product of two such sums over m), so the two
covariances differ by E with ||E||_2 <= 3 * 6 (m + 8) u T0; by Davis-Kahan the normals differ, up to sign, by at most
delta = 4 ||E||_2 / (l2 - l1) = 72 (m + 8) u kappa / gap, with gap the smallest relative eigen-gap and kappa the largest
T0 / (m trace) -- both measured by the ORACLE on the input.  C = mean n n' then moves by at most 2 delta per entry; det's
gradient is the cofactor matrix, whose nine entries are bounded by 1 for a C with trace 1, so |d det| <= 18 delta; trace stays
1; the smallest eigenvalue moves by at most ||dC||_2 <= 6 delta.  The bar: normals within delta + 1e-12 up to sign, every
response within 18 delta + 1e-12.  On the four inputs delta <= 6.4e-11 (gap >= 5.6e-2, kappa <= 2.1, m <= 713); measured:
normals within 5.6e-15, responses within 1.2e-16."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import harris_oracle as ho
from conftest import GOLDEN, ROOT
from usip_amd import baselines as bl

sys.path.insert(0, GOLDEN)
import make_baseline_walk_golden as golden  # noqa: E402

TOL = 1e-12
U = 1.1e-16


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def one(out):
    return tuple(a[0] for a in out)


@functools.lru_cache(maxsize=None)
def oracle(inp, response="harris", supplied=False):
    """the oracle's answer on one of the box inputs, computed once per session; nobody writes into it"""
    pc, analytic = ho.boxes(*inp, want_normals=True)
    return ho.harris(pc, normals=analytic if supplied else None, response=response)


def delta_of(o):
    return 72.0 * (o["m_max"] + 8) * U * o["kappa"] / o["gap"]


def against_oracle(got, o, neighbours=None):
    """got = (mask, response, members, normals) of ONE frame; o = the oracle's dict for the same input and arguments"""
    print("gap %.3e, threshold margin %.3e, tie margin %.3e, kappa %.2f, m <= %d, %d keypoints, %d at or above the threshold"
          % (o["gap"], o["thr"], o["tie"], o["kappa"], o["m_max"], o["mask"].sum(), o["above"]))
    assert o["gap"] > ho.MARGIN and o["thr"] > ho.MARGIN and o["tie"] > ho.MARGIN     # a condition on the input
    mask, res, members, normals = got
    assert np.array_equal(np.flatnonzero(mask), np.flatnonzero(o["mask"]))
    assert np.array_equal(members, o["members"])
    if neighbours is not None:
        assert np.array_equal(neighbours, o["neighbours"])
    estimated = o["neighbours"] is not None
    delta = delta_of(o) if estimated and np.isfinite(o["gap"]) else 0.0
    has = (o["normals"] != 0).any(1)                                    # (a supplied row without a normal stays as given)
    n = normals.T[has]
    nerr = np.minimum(np.abs(n - o["normals"][has]).max(1), np.abs(n + o["normals"][has]).max(1)).max() if has.any() else 0.0
    assert (normals.T[~has] == 0).all() or not estimated
    err = np.abs(res - o["response"]).max()
    print("normals: max error %.3e (bar %.3e); response: max error %.3e (bar %.3e)"
          % (nerr, delta + TOL, err, 18 * delta + TOL))
    assert nerr <= (delta + TOL if estimated else 0.0)                  # (supplied normals come back as given)
    assert err <= 18 * delta + TOL
    return o


# ---------------------------------------------------------------------------------------------------- inputs, shared with the GPU tests
SMALL = {1: (5, 0.2), 2: (6, 0.2), 3: (7, 0.2), 255: (8, 2.0), 256: (9, 2.0), 257: (10, 2.0)}      # n -> (seed, h) of a box


def small_frame(n):
    return ho.boxes(SMALL[n][0], n, SMALL[n][1])


def ragged_batch():
    """B = 3 frames of N = 300 slots with 257 / 256 / 1 live points; the dead slots hold NaN, which nothing may read into a
    result."""
    pc = np.stack([ho.boxes(11, 300, 2.0), ho.boxes(12, 300, 2.0), ho.boxes(13, 300, 2.0)])
    count = np.array([257, 256, 1], np.int32)
    for b in range(3):
        pc[b, :, count[b]:] = np.nan
    return pc, count


def noisy_normals(inp, seed=5):
    """supplied normals that are not unit vectors: the analytic face normals plus 0.05 N(0,1) per component, float32 -- no
    two points share a normal, so no two responses are equal but for rounding"""
    pc, analytic = ho.boxes(*inp, want_normals=True)
    return pc, (analytic + 0.05 * np.random.RandomState(seed).normal(size=analytic.shape)).astype(np.float32)


def degenerate_frames():
    """name -> pc f32 [3,n]"""
    t = np.arange(12, dtype=np.float32) / 8
    zero = np.zeros_like(t)
    rng = np.random.RandomState(4)
    plane = np.stack([rng.uniform(-3, 3, 400), rng.uniform(-3, 3, 400), 0.5 + 0.01 * rng.normal(size=400)]).astype(np.float32)
    return {
        "coincident": np.tile(np.array([[1.5], [-2.0], [0.25]], np.float32), (1, 10)),
        "line_x": np.stack([t, zero, zero]), "line_y": np.stack([zero, t, zero]), "line_z": np.stack([zero, zero, t]),
        "isolated": np.stack([np.arange(9, dtype=np.float32) * 10, zero[:9], zero[:9]]),
        "plane": plane,
        "duplicates": np.repeat(ho.boxes(6, 150, 1.0), 2, axis=1),
    }


def check_degenerate(name, pc, mask, res, members, normals, neighbours):
    n = pc.shape[1]
    if name == "coincident":
        # a zero trace: normal_from's (0, 0, 1), flipped towards the origin because z = 0.25 > 0; C = n n' has det 0
        assert (neighbours == n).all() and (members == n).all()
        assert (normals == np.array([[0.0], [0.0], [-1.0]])).all() and (res == 0).all() and not mask.any()
    elif name in ("line_x", "line_y", "line_z"):
        # the first of the two zero eigenvalues: one and the same axis-parallel normal for every point, det 0
        axis = "xyz".index(name[-1])
        assert (neighbours >= 8).all() and np.array_equal(members, neighbours)
        assert (normals[axis] == 0).all() and (np.abs(normals).sum(0) == 1).all() and (normals == normals[:, :1]).all()
        assert (res == 0).all() and not mask.any()
    elif name == "isolated":
        assert (neighbours == 1).all() and (normals == 0).all() and (res == 0).all() and (members == 0).all() and not mask.any()
    elif name == "plane":
        assert (neighbours >= 3).all() and np.array_equal(members, neighbours)
        assert (np.abs(normals[2]) > 0.99).all() and (normals[2] < 0).all()     # flipped towards the origin below the plane
        assert (res < ho.THRESHOLD).all() and not mask.any()
    elif name == "duplicates":
        assert np.array_equal(bits(res[0::2]), bits(res[1::2])) and np.array_equal(bits(normals[:, 0::2]), bits(normals[:, 1::2]))
        assert np.array_equal(mask[0::2], mask[1::2]) and mask.sum() >= 2      # equal responses do not suppress each other
    else:
        raise KeyError(name)


def twin(pc, count=None, num_threads=4, **kw):
    """-> (mask, response, members, normals), neighbours; neighbours is None with supplied normals"""
    out = bl.harris_keypoints_cpu(pc, count, num_threads=num_threads, **kw)
    nb = None
    if kw.get("normals") is None:
        nrm, nb = bl.harris_normals_cpu(pc, count, kw.get("radius", 1.0), kw.get("min_neighbors", 3), num_threads)
        assert np.array_equal(bits(nrm), bits(out[3]))
    return out, nb


# ---------------------------------------------------------------------------------------------------- the detector
@pytest.mark.parametrize("inp", ho.INPUTS)
def test_host_twin_against_the_oracle(inp):
    pc = ho.boxes(*inp)
    out, nb = twin(pc[None])
    o = against_oracle(one(out), oracle(inp), nb[0])
    assert o["mask"].sum() == ho.KEYPOINTS[inp]
    assert np.abs(np.linalg.norm(out[3][0], axis=0) - 1).max() < 1e-12  # every point of these inputs has a normal


@pytest.mark.parametrize("response", ho.METHODS[1:])
def test_other_responses(response):
    inp = ho.INPUTS[1]
    pc = ho.boxes(*inp)
    out, _ = twin(pc[None], response=response)
    o = against_oracle(one(out), oracle(inp, response))
    assert o["mask"].any()
    if response != "tomasi":                                            # trace = 1: det in another guise
        assert np.abs(out[1][0] - oracle(inp)["response"]).max() < 1e-9


@pytest.mark.parametrize("inp", ho.INPUTS[:3])
def test_supplied_analytic_normals(inp):
    """The face normals the generator knows, rotated with the cloud.  Every point of a face carries the same float32 normal, so
    points whose members split over the faces in the same proportions have responses that are equal but for rounding; the
    fourth input has such a pair within reach of each other (the oracle's tie margin says so: 2e-16) and is supplied with
    noisy normals below instead."""
    pc, analytic = ho.boxes(*inp, want_normals=True)
    out, _ = twin(pc[None], normals=analytic[None])
    o = against_oracle(one(out), oracle(inp, supplied=True))
    assert o["mask"].any() and np.array_equal(out[3][0], analytic.astype(np.float64))


def test_supplied_normals_are_used_as_given():
    """not renormalised; a row with a non-finite component or three zeros has no normal"""
    inp = ho.INPUTS[3]
    pc, nrm = noisy_normals(inp)
    nrm[:, 7] = 0.0
    nrm[1, 8] = np.nan
    nrm[2, 9] = np.inf
    out, _ = twin(pc[None], normals=nrm[None])
    o = against_oracle(one(out), ho.harris(pc, normals=nrm))
    assert (out[1][0, 7:10] == 0).all() and (out[2][0, 7:10] == 0).all() and not out[0][0, 7:10].any()
    assert o["mask"].any() and np.abs(np.linalg.norm(nrm[:, 10:].astype(np.float64), axis=0) - 1).max() > 0.05


@pytest.mark.parametrize("n", sorted(SMALL))
def test_small_frames(n):
    pc = small_frame(n)
    out, nb = twin(pc[None])
    against_oracle(one(out), ho.harris(pc), nb[0])
    if n < 3:
        assert (nb == n).all() and (out[3] == 0).all() and (out[1] == 0).all() and (out[2] == 0).all() and not out[0].any()
    if n == 3:
        assert (nb == 3).all() and (out[2] == 3).all() and not out[0].any()      # one plane through three points


def test_ragged_count():
    pc, count = ragged_batch()
    (mask, res, members, normals), nb = twin(pc, count, num_threads=2)
    for b, n in enumerate(count):
        (m1, r1, k1, n1), nb1 = twin(np.ascontiguousarray(pc[b:b + 1, :, :n]))
        assert np.array_equal(mask[b, :n], m1[0]) and np.array_equal(bits(res[b, :n]), bits(r1[0]))
        assert np.array_equal(members[b, :n], k1[0]) and np.array_equal(bits(normals[b, :, :n]), bits(n1[0]))
        assert np.array_equal(nb[b, :n], nb1[0])
        assert not mask[b, n:].any() and (res[b, n:] == 0).all() and (members[b, n:] == 0).all()
        assert (normals[b, :, n:] == 0).all() and (nb[b, n:] == 0).all()
        against_oracle((m1[0], r1[0], k1[0], n1[0]), ho.harris(pc[b, :, :n]), nb1[0])
    assert mask[0].sum() > 0 and mask[1].sum() > 0


@pytest.mark.parametrize("name", sorted(degenerate_frames()))
def test_degenerate_frames(name):
    pc = degenerate_frames()[name]
    out, nb = twin(pc[None])
    check_degenerate(name, pc, *one(out), nb[0])


@pytest.mark.parametrize("inp", [ho.INPUTS[0], ho.INPUTS[1]])
def test_axis_permutation_keeps_the_keypoints(inp):
    """x -> z -> y -> x is exact in float32: another sort axis, another order of the sums, the same index set."""
    pc = ho.boxes(*inp)
    turned = np.ascontiguousarray(pc[[1, 2, 0]])
    a, b = one(twin(pc[None])[0]), one(twin(turned[None])[0])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[0].sum() == ho.KEYPOINTS[inp]
    assert not np.array_equal(bits(a[1]), bits(b[1]))                   # (the sums did take another order)
    assert np.abs(a[1] - b[1]).max() <= 18 * delta_of(oracle(inp)) + TOL


def test_thread_count_does_not_change_a_bit():
    pc, count = ragged_batch()
    a, b = twin(pc, count, num_threads=1)[0], twin(pc, count, num_threads=4)[0]
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


def test_bad_arguments_raise():
    pc = ho.boxes(0, 16, 1.0)[None]
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(threshold=-0.1), dict(min_neighbors=0), dict(response="moravec"),
               dict(normals=np.zeros((1, 3, 16), np.float64)), dict(normals=np.zeros((1, 3, 15), np.float32))):
        with pytest.raises((RuntimeError, ValueError)):
            bl.harris_keypoints_cpu(pc, **kw)
    with pytest.raises(ValueError):
        bl.harris_keypoints_cpu(pc[0])                                  # not [B,3,N]
    with pytest.raises(ValueError):
        bl.harris_keypoints_cpu(pc, count=np.array([1, 2], np.int32))
    with pytest.raises(RuntimeError):
        bl.harris_normals_cpu(np.zeros((1, 3, (1 << 20) + 1), np.float32))          # N <= NMAX
    with pytest.raises(ValueError):
        bl.HarrisDetector(radius=0.0)
    with pytest.raises(ValueError):
        bl.HarrisDetector(response="moravec")
    assert bl.HARRIS_DEFAULTS == dict(radius=1.0, threshold=0.001, response="harris", min_neighbors=3)


# ---------------------------------------------------------------------------------------------------- the bits pinned at one commit
@pytest.mark.parametrize("num_threads", [1, 3])
@pytest.mark.parametrize("name", sorted(golden.CASES))
def test_twin_equals_the_bits_pinned_before_the_shared_frame_loop(name, num_threads):
    """tests/golden/make_baseline_walk_golden.py: what this twin computed before csrc/frames_host.h and
    csrc/ascending_walk.h, every entry =="""
    golden.check("harris", name, golden.harris_host(name, num_threads), "host twin, %d threads" % num_threads)


# ---------------------------------------------------------------------------------------------------- the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "harris_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# a host compiler: g++ or clang++ where there is one, otherwise the clang++ beside hipcc, which every build here needs anyway
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/harris_cpu.cpp: random frames, counts in and out of range, ties,
    non-finite coordinates and normals.  It links nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "harris_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "harris_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
