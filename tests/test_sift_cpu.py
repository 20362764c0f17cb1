"""The SIFT3D baseline detector's host twin (csrc/sift_cpu.cpp over csrc/sift_math.h) against the independent oracle
(tests/sift_oracle.py), its degenerate frames with explicit expectations, the selection rule, and a stand-alone sanitizer
build.  The device is held to this twin bit for bit in tests/test_sift_gpu.py, which borrows the inputs.

The bar against the oracle is derived, not fitted.  With u = 1.1e-16, m the members of a query at the widest
scale, F the largest |f| of the octave cloud and E the largest relative error of sift_exp against numpy.exp on [-4.5, 0]
(measured below on 2 000 001 points: 2.3e-16), num_s and den_s of either side carry a relative perturbation of at most
E + (m + 2) u of sum |f_j| w_j and sum w_j (one rounding of the weight's argument chain folded into E's neighbour, m - 1
additions, one product), so |dG| <= 2 (E + (m + 2) u) F and a DoG entry moves by at most twice that: bound = 4 (E + (m + 2) u)
F, computed by the ORACLE per octave from its own m and F (at most 3.6e-13 on the inputs here; measured: 2.7e-15).  Every
oracle test first asserts, as a condition on the input, that the two absolute margins (|DoG| from min_contrast; a DoG value
from every other value it is compared with) exceed 100 x bound and the two relative ones (a d2 from a 9 sigma^2; the 25th from
the 26th nearest) exceed 1e-9.  Then: octave clouds bit-equal, 25-lists identical, dog within the bound, keypoint index set and
scale indices identical."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sift_oracle as so
from conftest import GOLDEN, ROOT
from usip_amd import baselines as bl

sys.path.insert(0, GOLDEN)
import make_baseline_walk_golden as golden  # noqa: E402

U = so.U
SMALL = dict(min_scale=0.5, n_octaves=2, n_scales_per_octave=3, min_contrast=0.02)


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


@functools.lru_cache(maxsize=None)
def exp_error():
    """E: sift_exp against numpy.exp on a dense grid over [-4.5, 0], relative"""
    x = np.linspace(-4.5, 0.0, 2000001)
    want = np.exp(x)
    return float((np.abs(bl.sift_exp_cpu(x) - want) / want).max())


@functools.lru_cache(maxsize=None)
def oracle(name, supplied=False, scales=None, octaves=None):
    """the oracle's answer on one of the terrain inputs, computed once per session; nobody writes into it"""
    pc = so.cloud_of(name)
    par = dict(so.INPUTS[name][1])
    if scales is not None:
        par["n_scales_per_octave"] = scales
    if octaves is not None:
        par["n_octaves"] = octaves
    return so.sift(pc, so.reflectance(pc) if supplied else 2, exp_error=exp_error(), **par)


def twin(pc, count=None, field="z", num_threads=4, **par):
    """pc [B,3,N] -> bl.sift_keypoints_cpu's five results"""
    return bl.sift_keypoints_cpu(pc, count, field=field, want_octaves=True, num_threads=num_threads, **par)


def against_oracle(octaves, want, b=0):
    """octaves: the per-octave tuples of the twin (or the device, on the host); want: the oracle's list for frame b"""
    for o, (cloud, fld, cnt, dog, idx, mask, sidx) in enumerate(octaves):
        if o >= len(want):                                              # behind the 25-point rule: nothing
            assert cnt[b] < so.NEAREST and not mask[b].any() and (dog[b] == 0).all()
            continue
        w = want[o]
        n = w["cloud"].shape[1]
        assert cnt[b] == n
        assert np.array_equal(bits(cloud[b, :, :n]), bits(w["cloud"])) and np.array_equal(bits(fld[b, :n]), bits(w["field"]))
        assert (cloud[b, :, n:] == 0).all() and (fld[b, n:] == 0).all()
        if n < so.NEAREST:
            assert not mask[b].any() and (dog[b] == 0).all() and (idx[b] == 0).all() and (sidx[b] == 0).all()
            continue
        print("octave %d: %d rows, %d keypoints, m <= %d, bound %.2e; margins: d2 %.2e, 25th/26th %.2e, contrast %.2e, ties "
              "%.2e; |DoG| <= %.2f" % (o, n, w["mask"].sum(), w["m_max"], w["bound"], w["d2_margin"], w["gap_margin"],
                                        w["contrast_margin"], w["tie_margin"], w["dog_max"]))
        assert w["contrast_margin"] > 100 * w["bound"] and w["tie_margin"] > 100 * w["bound"]       # conditions on the input
        assert w["d2_margin"] > 1e-9 and w["gap_margin"] > 1e-9
        assert np.array_equal(idx[b, :n], w["idx"])
        err = np.abs(dog[b, :, :n] - w["dog"]).max()
        print("          dog: max error %.3e" % err)
        assert err <= w["bound"]
        assert np.array_equal(np.flatnonzero(mask[b]), np.flatnonzero(w["mask"]))
        assert np.array_equal(sidx[b, :n], w["scale"])
        assert (dog[b, :, n:] == 0).all() and (idx[b, n:] == 0).all() and (sidx[b, n:] == 0).all()


def frame_of(octave, b, n, behind=False):
    """frame b of one octave's (cloud, field, count, dog, idx, mask, scale_index), cut to n slots -- or the slots behind them"""
    cloud, fld, cnt, dog, idx, mask, sidx = octave
    s = slice(n, None) if behind else slice(0, n)
    return (cloud[b:b + 1, :, s], fld[b:b + 1, s], cnt[b:b + 1] * (0 if behind else 1), dog[b:b + 1, :, s], idx[b:b + 1, s],
            mask[b:b + 1, s], sidx[b:b + 1, s])


# ---------------------------------------------------------------------------------------------------- inputs, shared with the GPU tests
def ragged_batch():
    """B = 3 frames of N = 300 slots with 257 / 256 / 1 live points; the dead slots hold NaN, which nothing may read into a
    result."""
    pc = np.stack([np.ascontiguousarray(so.terrain(11 + b, 300, 8, 1.0).T) for b in range(3)])
    count = np.array([257, 256, 1], np.int32)
    for b in range(3):
        pc[b, :, count[b]:] = np.nan
    return pc, count


def lattice(n, seed=2):
    """n <= 49 points, one per cell of a 7 x 7 grid of leaf 0.5, with a height of their own: an octave cloud of exactly n rows"""
    g = np.random.default_rng(seed)
    i = np.arange(n)
    return np.stack([(i // 7) * 0.5 + g.uniform(0.1, 0.4, n), (i % 7) * 0.5 + g.uniform(0.1, 0.4, n),
                     g.uniform(0.05, 0.45, n)]).astype(np.float32)


def degenerate_frames():
    """name -> (pc f32 [3,n], field, parameters)"""
    g = np.random.default_rng(4)
    plane = np.stack([g.uniform(-6, 6, 1500), g.uniform(-6, 6, 1500), 0.7 + 0.01 * g.standard_normal(1500)]).astype(np.float32)
    cell = g.uniform(0.01, 0.49, (3, 100)).astype(np.float32)
    a = so.cloud_of("C")
    return {
        "plane": (plane, "z", SMALL),
        "constant": (plane, np.full(1500, 0.7, np.float32), SMALL),
        "single": (np.array([[1.5], [-2.0], [0.25]], np.float32), "z", SMALL),
        "one_cell": (cell, "z", SMALL),
        "coincident": (np.tile(np.array([[1.3], [-2.1], [0.2]], np.float32), (1, 40)), "x", SMALL),
        "duplicates": (np.repeat(a, 2, axis=1), "z", so.INPUTS["C"][1]),
        "rows24": (lattice(24), "z", dict(SMALL, n_octaves=1, min_contrast=0.0)),
        "rows25": (lattice(25), "z", dict(SMALL, n_octaves=1, min_contrast=0.0)),
    }


def check_degenerate(name, pc, out):
    cand, mask, scale, counts, octaves = out
    cloud, fld, cnt, dog, idx, m0, sidx = octaves[0]
    n = pc.shape[1]
    if name in ("plane", "constant"):
        # heights (a field) that differ by noise only: every |DoG| is far below the contrast
        assert counts[0, 0] > 500 and counts[0, 1] >= 25 and not mask.any() and (scale == 0).all()
        # a constant field f: num = f * den but for the roundings of at most n - 1 additions and a product each, so
        # |G - f| <= (n + 2) u f on either side of a difference
        assert np.abs(dog).max() < (0.01 if name == "plane" else 2 * (n + 2) * U * 0.7)
    elif name == "single":
        assert counts.tolist() == [[1, 1]] and np.array_equal(cloud[0, :, 0], pc[:, 0]) and fld[0, 0] == pc[2, 0]
        assert not mask.any() and (dog == 0).all() and (idx == 0).all()
    elif name == "one_cell":
        want = (np.cumsum(pc.astype(np.float64), axis=1)[:, -1] / n).astype(np.float32)     # (cumsum adds one at a time)
        assert counts.tolist() == [[1, 1]] and np.array_equal(cloud[0, :, 0], want) and fld[0, 0] == want[2]
        assert (cloud[0, :, 1:] == 0).all() and not mask.any()
    elif name == "coincident":
        assert counts.tolist() == [[1, 1]] and np.array_equal(cloud[0, :, 0], pc[:, 0]) and fld[0, 0] == pc[0, 0]
    elif name == "duplicates":                                          # they merge: the cells of the cloud without them
        single = oracle("C")
        assert counts[0].tolist() == [single[0]["cloud"].shape[1], single[1]["cloud"].shape[1]]
        assert np.abs(cloud[0, :, :counts[0, 0]] - single[0]["cloud"]).max() < 1e-6
        assert np.array_equal(np.flatnonzero(m0[0]), np.flatnonzero(single[0]["mask"]))
    elif name == "rows24":
        assert counts.tolist() == [[24]] and not mask.any() and (dog == 0).all() and (idx == 0).all() and (sidx == 0).all()
        assert np.array_equal(np.sort(cloud[0, 0, :24]), np.sort(pc[0]))
    elif name == "rows25":
        assert counts.tolist() == [[25]] and np.abs(dog).max() > 1e-4
        assert np.array_equal(np.sort(idx[0], axis=1), np.tile(np.arange(25, dtype=np.int32), (25, 1)))
        assert np.array_equal(idx[0, :, 0], np.arange(25))              # d2 = 0: the row itself comes first
        against_oracle(octaves, so.sift(pc, 2, exp_error=exp_error(), **degenerate_frames()[name][2]))
    else:
        raise KeyError(name)


def staggered_batch():
    """B = 3 frames whose octaves end at different depths under the 25-point rule (4 octaves asked for)"""
    frames = [so.terrain(21, 60, 3, 0.5), so.terrain(3, 600, 12, 1.0), so.terrain(22, 900, 30, 1.0)]
    N = 900
    pc = np.full((3, 3, N), np.nan, np.float32)
    for b, f in enumerate(frames):
        pc[b, :, :len(f)] = f.T
    return pc, np.array([len(f) for f in frames], np.int32), dict(SMALL, n_octaves=4)


def quantised(name="A"):
    """the terrain with x on a lattice of 2^-10, so that x + 8 is exact in float32"""
    pc = so.cloud_of(name).copy()
    pc[0] = np.round(pc[0] * 1024) / 1024
    return pc


# ---------------------------------------------------------------------------------------------------- the detector
def test_sift_exp_against_numpy():
    e = exp_error()
    print("E = %.3e" % e)
    assert e < 4 * U                                                    # DESIGN 8l quotes 2.3e-16
    assert bl.sift_exp_cpu(np.zeros(1))[0] == 1.0


@pytest.mark.parametrize("name", sorted(so.INPUTS))
def test_host_twin_against_the_oracle(name):
    want = oracle(name)
    out = twin(so.cloud_of(name)[None], **so.INPUTS[name][1])
    against_oracle(out[4], want)
    # what the numpy prototype of the contract saw (the table of the feature's issue)
    assert tuple(w["cloud"].shape[1] for w in want) == so.CLOUDS[name]
    assert tuple(int(w["mask"].sum()) for w in want) == so.KEYPOINTS[name]
    if name in so.MEMBERS:
        assert max(w["m_max"] for w in want) == so.MEMBERS[name]
    N = out[0].shape[2] // len(want)
    for o, w in enumerate(want):                                        # the flat results are the octaves side by side
        n = w["cloud"].shape[1]
        assert out[3][0, o] == n and np.array_equal(out[0][0, :, o * N:o * N + n], w["cloud"])
        assert np.array_equal(out[2][0, o * N:o * N + n], np.where(w["mask"], w["sigma"][w["scale"]], 0.0))


def test_supplied_field():
    pc = so.cloud_of("A")
    out = twin(pc[None], field=so.reflectance(pc)[None], **so.INPUTS["A"][1])
    want = oracle("A", supplied=True)
    against_oracle(out[4], want)
    assert not np.array_equal(want[0]["field"], want[0]["cloud"][2]) and sum(int(w["mask"].sum()) for w in want) > 0


def test_one_scale_per_octave():
    out = twin(so.cloud_of("C")[None], **dict(so.INPUTS["C"][1], n_scales_per_octave=1))
    want = oracle("C", scales=1)
    against_oracle(out[4], want)
    assert out[4][0][3].shape[1] == 3 and set(np.unique(out[4][0][6])) <= {0, 1}


def test_the_25_point_rule_ends_the_octaves():
    out = twin(so.cloud_of("C")[None], **dict(so.INPUTS["C"][1], n_octaves=4))
    want = oracle("C", octaves=4)
    assert [w["cloud"].shape[1] for w in want] == [390, 155, 45, 23]    # the fourth cloud is too small
    against_oracle(out[4], want)
    assert out[3][0].tolist() == [390, 155, 45, 23] and not out[4][3][5].any() and (out[4][3][3] == 0).all()
    assert out[1].sum() == sum(so.KEYPOINTS["C"]) + int(want[2]["mask"].sum()) and out[4][2][5].any()


@pytest.mark.parametrize("name", sorted(degenerate_frames()))
def test_degenerate_frames(name):
    pc, field, par = degenerate_frames()[name]
    out = twin(pc[None], field=field if isinstance(field, str) else field[None], **par)
    check_degenerate(name, pc, out)


def test_translation_by_whole_leaves_keeps_the_index_set():
    pc = quantised()
    moved = pc.copy()
    moved[0] += 8.0                                                     # 16 leaves of octave 0, 8 of octave 1; exact
    assert np.array_equal(moved[0].astype(np.float64) - 8.0, pc[0].astype(np.float64))
    a, b = twin(pc[None], **so.INPUTS["A"][1]), twin(moved[None], **so.INPUTS["A"][1])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1]) and a[1].sum() > 0
    for oa, ob in zip(a[4], b[4]):
        assert np.array_equal(oa[6], ob[6]) and np.array_equal(oa[4], ob[4])
        assert np.array_equal(bits(oa[0][:, 1:]), bits(ob[0][:, 1:]))    # y and z of the centroids: the same sums


def test_ragged_count_and_staggered_octaves():
    for pc, count, par in (ragged_batch() + (SMALL,), staggered_batch()):
        out = twin(pc, count, num_threads=2, **par)
        for b, n in enumerate(count):
            one = twin(np.ascontiguousarray(pc[b:b + 1, :, :n]), **par)
            for ob, o1 in zip(out[4], one[4]):
                for x, y, z in zip(frame_of(ob, b, n), o1, frame_of(ob, b, n, behind=True)):
                    assert np.array_equal(bits(x), bits(y)) and (z == 0).all()
            against_oracle(one[4], so.sift(pc[b, :, :n], 2, exp_error=exp_error(), **par))
    pc, count, par = staggered_batch()
    depth = [(twin(pc, count, **par)[3][b] >= 25).sum() for b in range(3)]
    print("octaves with at least 25 rows:", depth)
    assert len(set(depth)) == 3


def test_thread_count_does_not_change_a_bit():
    pc, count, par = staggered_batch()
    a, b = twin(pc, count, num_threads=1, **par), twin(pc, count, num_threads=5, **par)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(bits(x), bits(y))
    for oa, ob in zip(a[4], b[4]):
        for x, y in zip(oa, ob):
            assert np.array_equal(bits(x), bits(y))


def test_bad_arguments_raise():
    pc = so.cloud_of("C")[None]
    for kw in (dict(min_scale=0.0), dict(min_scale=-1.0), dict(min_scale=float("nan")), dict(min_scale=float("inf")),
               dict(min_contrast=-0.1), dict(min_contrast=float("nan")), dict(n_octaves=0), dict(n_octaves=9),
               dict(n_scales_per_octave=0), dict(n_scales_per_octave=9), dict(field="w"),
               dict(field=np.zeros((1, 600), np.float64)), dict(field=np.zeros((1, 599), np.float32))):
        with pytest.raises((RuntimeError, ValueError)):
            bl.sift_keypoints_cpu(pc, **kw)
    with pytest.raises(ValueError):
        bl.sift_keypoints_cpu(pc[0])                                    # not [B,3,N]
    with pytest.raises(ValueError):
        bl.sift_keypoints_cpu(pc, count=np.array([1, 2], np.int32))
    # the library's own limits (USIP_EINVAL)
    cloud, fld, cnt = bl.sift_octave_cpu(pc, "z", None, 0.5)
    good = bl.sift_sigma2(0.5, 3)
    for s2 in (good[:3], np.r_[good, good, good[-1]][:12], good[::-1], np.r_[0.0, good[1:]], np.r_[good[:-1], np.inf],
               np.r_[good[:-1], np.nan]):
        with pytest.raises(RuntimeError):
            bl.sift_dog_cpu(cloud, fld, cnt, s2)
    dog, idx = bl.sift_dog_cpu(cloud, fld, cnt, good), bl.sift_nearest_cpu(cloud, cnt)
    for bad in (-1.0, float("nan")):
        with pytest.raises(RuntimeError):
            bl.sift_extrema_cpu(dog, idx, cnt, bad)
    with pytest.raises(RuntimeError):
        bl.sift_extrema_cpu(dog[:, :2], idx, cnt, 0.1)                   # S = 3
    for leaf in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            bl.sift_octave_cpu(pc, "z", None, leaf)
    with pytest.raises(RuntimeError):
        bl.sift_nearest_cpu(np.zeros((1, 3, (1 << 20) + 1), np.float32), None)      # N <= NMAX
    with pytest.raises(ValueError):
        bl.SiftDetector(min_scale=0.0)
    with pytest.raises(ValueError):
        bl.SiftDetector(n_scales_per_octave=9)
    with pytest.raises(ValueError):
        bl.SiftDetector(field="w")
    # save_keypoints.py:57-61
    assert bl.SIFT_DEFAULTS == dict(min_scale=0.5, n_octaves=4, n_scales_per_octave=8, min_contrast=0.1, field="z")


def test_cells_outside_the_key_range_and_non_finite_rows_are_dropped():
    pc = lattice(30)
    pc[0, 3], pc[1, 4], pc[2, 5] = np.nan, np.inf, -np.inf
    pc[0, 6], pc[0, 7] = 0.5 * (1 << 20), -0.5 * (1 << 20) - 0.25      # cell 2^20 (outside) and cell -2^20 - 1 (outside)
    pc[0, 8] = -0.5 * (1 << 20)                                         # cell -2^20: the lowest inside
    cloud, fld, cnt = bl.sift_octave_cpu(pc[None], "z", None, 0.5)
    assert cnt.tolist() == [25] and np.array_equal(cloud[0, :, 0], pc[:, 8]) and np.isfinite(cloud).all()


def test_walk_radius_covers_the_widest_scale():
    for base in (0.5, 1.0, 0.3, 4.0, 0.7):
        for k in range(1, 9):
            s2 = bl.sift_sigma2(base, k)
            r = bl.sift_walk_radius(s2)
            assert r * r >= 9.0 * s2[-1] and np.nextafter(r, 0.0) ** 2 < 9.0 * s2[-1] * (1 + 1e-15) and len(s2) == k + 3


# ---------------------------------------------------------------------------------------------------- the bits pinned at one commit
@pytest.mark.parametrize("num_threads", [1, 3])
@pytest.mark.parametrize("name", sorted(golden.CASES))
def test_twin_equals_the_bits_pinned_before_the_shared_frame_loop(name, num_threads):
    """tests/golden/make_baseline_walk_golden.py: what this twin computed before csrc/frames_host.h and
    csrc/ascending_walk.h, every entry =="""
    golden.check("sift", name, golden.sift_host(name, num_threads), "host twin, %d threads" % num_threads)


# ---------------------------------------------------------------------------------------------------- the selection
def test_selection_rule():
    pc = so.cloud_of("A")[None]
    cand, mask, scale, counts = bl.sift_keypoints_cpu(pc, **so.INPUTS["A"][1])
    found = int(mask.sum())
    assert found == 16
    M, N = cand.shape[2], pc.shape[2]
    u = bl._draws(1, M + N, 3, [7]).numpy()[0]
    # more candidates than num: the `num` keypoints with the smallest draws, in that order
    kp, cnt, order = bl.select_candidates_cpu(pc, None, cand, mask, 5, True, 3, [7], want_index=True)
    slots = np.flatnonzero(mask[0])
    want = slots[np.argsort(u[slots], kind="stable")][:5]
    assert cnt.tolist() == [5] and np.array_equal(order[0], want) and np.array_equal(kp[0], cand[0][:, want])
    # fewer: every keypoint first, then cloud points pad; nothing repeats
    kp, cnt, order = bl.select_candidates_cpu(pc, None, cand, mask, 64, True, 3, [7], want_index=True)
    assert cnt.tolist() == [64] and np.array_equal(np.sort(order[0, :found]), slots) and (order[0, found:] >= M).all()
    assert len(set(order[0].tolist())) == 64
    pad = order[0, found:] - M
    assert np.array_equal(pad, np.argsort(u[M:], kind="stable")[:64 - found]) and np.array_equal(kp[0][:, found:], pc[0][:, pad])
    # without ensure: the keypoints only; the slots beyond count hold the first pick
    kp, cnt, order = bl.select_candidates_cpu(pc, None, cand, mask, 64, False, 3, [7], want_index=True)
    assert cnt.tolist() == [found] and (order[0, found:] == order[0, 0]).all() and np.array_equal(np.sort(order[0, :found]), slots)
    # none found: with ensure cloud points only, without the frame's point 0 with count 1
    none = np.zeros_like(mask)
    kp, cnt, order = bl.select_candidates_cpu(pc, None, cand, none, 8, True, 3, [7], want_index=True)
    assert cnt.tolist() == [8] and (order >= M).all()
    kp, cnt, order = bl.select_candidates_cpu(pc, None, cand, none, 8, False, 3, [7], want_index=True)
    assert cnt.tolist() == [1] and (order == M).all() and np.array_equal(kp[0], np.repeat(pc[0][:, :1], 8, axis=1))
    # a ragged frame: dead cloud points never pad; fewer points than num
    count = np.array([3], np.int32)
    kp, cnt, order = bl.select_candidates_cpu(pc, count, cand, none, 8, True, 3, [7], want_index=True)
    assert cnt.tolist() == [3] and set(order[0, :3].tolist()) == {M, M + 1, M + 2} and (order[0, 3:] == order[0, 0]).all()
    # another frame id draws other numbers
    other = bl.select_candidates_cpu(pc, None, cand, mask, 5, True, 3, [8], want_index=True)[2]
    assert not np.array_equal(other[0], want)
    with pytest.raises(ValueError):
        bl.select_candidates_cpu(pc, None, cand, mask, 0)


# ---------------------------------------------------------------------------------------------------- the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "sift_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# a host compiler: g++ or clang++ where there is one, otherwise the clang++ beside hipcc, which every build here needs anyway
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/sift_cpu.cpp: random frames, counts in and out of range, ties, non-finite
    coordinates, wrong neighbour lists.  It links nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "sift_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "sift_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
