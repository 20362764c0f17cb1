"""The ISS baseline detector's host twin (csrc/iss_cpu.cpp over csrc/iss_math.h) against the independent oracle
(tests/iss_oracle.py), its degenerate frames with explicit expectations, and the keypoint-count rule of
usip_amd/baselines.py.  The device is held to this twin bit for bit in tests/test_iss_gpu.py, which borrows the inputs.

Bars against the oracle, valid where no decision sits on a threshold (both of the oracle's margins above 1e-9, asserted first
as a condition on the input): the keypoint index set and the neighbour counts identical; |saliency - oracle| <= 1e-12 *
trace(C) -- float64 rounding of a few hundred reordered sums (each within 1.1e-16 of the trace per term) and the Jacobi's
convergence after JACOBI_SWEEPS sweeps (far below that).  Measured on the four slab inputs: at most 2.2e-15 * trace."""
import sys

import numpy as np
import pytest

import iss_oracle as io
from conftest import GOLDEN
from usip_amd import baselines as bl

sys.path.insert(0, GOLDEN)
import make_baseline_walk_golden as golden  # noqa: E402

TOL = 1e-12


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def against_oracle(got, pc, **kw):
    """got = (mask, saliency, neighbours) of ONE frame; pc [3,n]"""
    o = io.iss(pc, **kw)
    print("gate margin %.3e, tie margin %.3e, %d keypoints" % (o["gate"], o["tie"], o["mask"].sum()))
    assert o["gate"] > io.MARGIN and o["tie"] > io.MARGIN               # a condition on the input
    mask, sal, nb = got
    assert np.array_equal(np.flatnonzero(mask), np.flatnonzero(o["mask"]))
    assert np.array_equal(nb, o["neighbours"])
    err = np.abs(sal - o["saliency"])
    print("saliency: max error %.3e of the trace" % (err / np.maximum(o["trace"], 1e-300)).max())
    assert (err <= TOL * o["trace"]).all()
    return o


def one(out):
    return tuple(a[0] for a in out)


# ---------------------------------------------------------------------------------------------------- inputs, shared with the GPU tests
SMALL = {1: (5, 1.0), 4: (6, 1.0), 5: (7, 0.5), 256: (8, 8.0), 257: (9, 8.0)}      # n -> (seed, h) of a slab cloud


def small_frame(n):
    """n = 5 is shrunk (exactly, by 1/4) so that its five points are each other's members: the smallest frame with a saliency"""
    pc = io.slab(SMALL[n][0], n, SMALL[n][1])
    return pc * np.float32(0.25) if n == 5 else pc


def ragged_batch():
    """B = 3 frames of N = 1000 slots with 1000 / 257 / 5 live points; the dead slots hold NaN, which nothing may read into
    a result."""
    pc = np.stack([io.slab(11, 1000, 12.0), io.slab(12, 1000, 8.0), io.slab(13, 1000, 0.7)])
    count = np.array([1000, 257, 5], np.int32)
    for b in range(3):
        pc[b, :, count[b]:] = np.nan
    return pc, count


def cluster(seed=4, n=40):
    """points on a 1/8 lattice, flattened along y and z: every coordinate and every translation by 64 is exact in float32"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, (3, n)) / 8.0 * np.array([[1.0], [0.5], [0.25]])).astype(np.float32)


def degenerate_frames():
    """name -> pc f32 [3,n]"""
    t = np.arange(12, dtype=np.float32) / 8
    zero = np.zeros_like(t)
    a = cluster()
    return {
        "coincident": np.tile(np.array([[1.5], [-2.0], [0.25]], np.float32), (1, 10)),
        "line_x": np.stack([t, zero, zero]), "line_y": np.stack([zero, t, zero]), "line_z": np.stack([zero, zero, t]),
        "isolated": np.stack([np.arange(9, dtype=np.float32) * 10, zero[:9], zero[:9]]),
        "two_clusters": np.concatenate((a, a + np.array([[64.0], [0.0], [0.0]], np.float32)), 1),
        "duplicates": np.repeat(cluster(6, 30), 2, axis=1),
    }


def check_degenerate(name, mask, sal, nb):
    if name in ("coincident", "line_x", "line_y", "line_z"):
        assert (nb == len(nb)).all()                                    # everything is within the radius
        assert (sal == 0).all() and not mask.any(), name
    elif name == "isolated":
        assert (nb == 1).all() and (sal == 0).all() and not mask.any()
    elif name == "two_clusters":
        h = len(nb) // 2
        assert np.array_equal(bits(sal[:h]), bits(sal[h:])) and np.array_equal(nb[:h], nb[h:])
        assert np.array_equal(mask[:h], mask[h:]) and mask[:h].sum() >= 1          # both maxima kept
    elif name == "duplicates":
        assert np.array_equal(bits(sal[0::2]), bits(sal[1::2]))         # equal saliencies do not suppress each other
        assert np.array_equal(mask[0::2], mask[1::2]) and mask.sum() >= 2


# ---------------------------------------------------------------------------------------------------- the detector
@pytest.mark.parametrize("inp", io.INPUTS)
def test_host_twin_against_the_oracle(inp):
    pc = io.slab(*inp)
    o = against_oracle(one(bl.iss_keypoints_cpu(pc[None], num_threads=4)), pc)
    assert o["mask"].sum() == io.KEYPOINTS[inp]


@pytest.mark.parametrize("inp", [io.INPUTS[1], io.INPUTS[2]])
def test_two_radii(inp):
    pc = io.slab(*inp)
    got = one(bl.iss_keypoints_cpu(pc[None], salient_radius=2.0, non_max_radius=1.0, num_threads=4))
    o = against_oracle(got, pc, salient_radius=2.0, non_max_radius=1.0)
    # the second radius is used: fewer rivals, but also fewer points with min_neighbors members -- another set
    assert not np.array_equal(o["mask"], io.iss(pc)["mask"]) and o["mask"].any()


@pytest.mark.parametrize("n", sorted(SMALL))
def test_small_frames(n):
    pc = small_frame(n)
    mask, sal, nb = one(bl.iss_keypoints_cpu(pc[None]))
    against_oracle((mask, sal, nb), pc)
    if n < 5:
        assert (sal == 0).all() and not mask.any()                      # nobody has min_neighbors = 5 members
    if n == 5:
        assert (nb == 5).all() and len(set(sal)) > 1                    # one scatter each, about its own point


def test_ragged_count():
    pc, count = ragged_batch()
    mask, sal, nb = bl.iss_keypoints_cpu(pc, count, num_threads=2)
    for b, n in enumerate(count):
        m1, s1, n1 = one(bl.iss_keypoints_cpu(np.ascontiguousarray(pc[b:b + 1, :, :n])))
        assert np.array_equal(mask[b, :n], m1) and np.array_equal(bits(sal[b, :n]), bits(s1)) and np.array_equal(nb[b, :n], n1)
        assert not mask[b, n:].any() and (sal[b, n:] == 0).all() and (nb[b, n:] == 0).all()
        against_oracle((m1, s1, n1), pc[b, :, :n])
    assert mask[0].sum() > 0 and mask[1].sum() > 0


@pytest.mark.parametrize("name", sorted(degenerate_frames()))
def test_degenerate_frames(name):
    pc = degenerate_frames()[name]
    check_degenerate(name, *one(bl.iss_keypoints_cpu(pc[None])))


@pytest.mark.parametrize("inp", [io.INPUTS[0], io.INPUTS[1]])
def test_axis_permutation_keeps_the_keypoints(inp):
    """x -> z -> y -> x is exact in float32: another sort axis, another order of the sums, the same index set."""
    pc = io.slab(*inp)
    turned = np.ascontiguousarray(pc[[1, 2, 0]])
    a, b = one(bl.iss_keypoints_cpu(pc[None])), one(bl.iss_keypoints_cpu(turned[None]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[0].sum() == io.KEYPOINTS[inp]
    assert not np.array_equal(bits(a[1]), bits(b[1]))                   # (the sums did take another order)
    assert np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(a[1]).max()


def test_thread_count_does_not_change_a_bit():
    pc, count = ragged_batch()
    a, b = bl.iss_keypoints_cpu(pc, count, num_threads=1), bl.iss_keypoints_cpu(pc, count, num_threads=4)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


def test_bad_arguments_raise():
    pc = io.slab(0, 16, 1.0)[None]
    for kw in (dict(salient_radius=0.0), dict(salient_radius=-1.0), dict(non_max_radius=0.0), dict(min_neighbors=0),
               dict(salient_radius=float("nan")), dict(non_max_radius=float("inf"))):
        with pytest.raises((RuntimeError, ValueError)):
            bl.iss_keypoints_cpu(pc, **kw)
    with pytest.raises(ValueError):
        bl.iss_keypoints_cpu(pc[0])                                     # not [B,3,N]
    with pytest.raises(ValueError):
        bl.iss_keypoints_cpu(pc, count=np.array([1, 2], np.int32))
    with pytest.raises(RuntimeError):
        bl.iss_saliency_cpu(np.zeros((1, 3, (1 << 20) + 1), np.float32))           # N <= NMAX
    with pytest.raises(ValueError):
        bl.IssDetector(salient_radius=0.0)
    with pytest.raises(ValueError):
        bl.select_keypoints_cpu(pc, np.zeros((1, 16), np.uint8), None, 0)
    with pytest.raises(ValueError):
        bl.select_keypoints_cpu(pc, np.zeros((1, 16), np.uint8), None, 4, frame_ids=[0, 1])


# ---------------------------------------------------------------------------------------------------- the bits pinned at one commit
@pytest.mark.parametrize("num_threads", [1, 3])
@pytest.mark.parametrize("name", sorted(golden.CASES))
def test_twin_equals_the_bits_pinned_before_the_shared_frame_loop(name, num_threads):
    """tests/golden/make_baseline_walk_golden.py: what this twin computed before csrc/frames_host.h and
    csrc/ascending_walk.h, every entry =="""
    golden.check("iss", name, golden.iss_host(name, num_threads), "host twin, %d threads" % num_threads)


# ---------------------------------------------------------------------------------------------------- the keypoint count
def selection_case():
    """B = 3 frames of 1000 slots: 40 keypoints / 7 keypoints / none, the last frame with 300 live points."""
    pc = np.stack([io.slab(21 + b, 1000, 12.0) for b in range(3)])
    rng = np.random.default_rng(9)
    mask = np.zeros((3, 1000), np.uint8)
    mask[0, rng.permutation(1000)[:40]] = 1
    mask[1, rng.permutation(1000)[:7]] = 1
    return pc, mask, np.array([1000, 1000, 300], np.int32)


def test_selection_rule():
    pc, mask, count = selection_case()
    kp, cnt, idx = bl.select_keypoints_cpu(pc, mask, count, 16, ensure=True, seed=3, frame_ids=[5, 6, 7], want_index=True)
    assert kp.shape == (3, 3, 16) and kp.dtype == np.float32 and cnt.dtype == np.int32 and cnt.tolist() == [16, 16, 16]
    for b in range(3):
        assert len(set(idx[b])) == 16 and (idx[b] < count[b]).all()
        assert np.array_equal(kp[b], pc[b][:, idx[b]])
    assert mask[0, idx[0]].all()                                        # more than num: a subset of the keypoints
    assert mask[1, idx[1, :7]].all() and not mask[1, idx[1, 7:]].any()  # fewer: all of them first, then other points
    assert sorted(idx[1, :7]) == sorted(np.flatnonzero(mask[1]))        # (so the padding never repeats a keypoint)
    # without ensure: what was found, at most num; the frame's point 0 when nothing was found
    kp2, cnt2, idx2 = bl.select_keypoints_cpu(pc, mask, count, 16, ensure=False, seed=3, frame_ids=[5, 6, 7], want_index=True)
    assert cnt2.tolist() == [16, 7, 1]
    assert np.array_equal(idx2[0], idx[0]) and np.array_equal(idx2[1, :7], idx[1, :7]) and (idx2[1, 7:] == idx2[1, 0]).all()
    assert (idx2[2] == 0).all() and np.array_equal(kp2[2], np.repeat(pc[2][:, :1], 16, 1))
    # the same (seed, frame_id): the same picks, whatever else is in the batch; another frame_id: other picks
    kp3, _, idx3 = bl.select_keypoints_cpu(pc[:1], mask[:1], count[:1], 16, seed=3, frame_ids=[5], want_index=True)
    assert np.array_equal(idx3[0], idx[0]) and np.array_equal(kp3[0], kp[0])
    _, _, idx4 = bl.select_keypoints_cpu(pc[:1], mask[:1], count[:1], 16, seed=3, frame_ids=[6], want_index=True)
    _, _, idx5 = bl.select_keypoints_cpu(pc[:1], mask[:1], count[:1], 16, seed=4, frame_ids=[5], want_index=True)
    assert not np.array_equal(idx4[0], idx[0]) and not np.array_equal(idx5[0], idx[0])
    # more asked for than there are live points: count says so, the rest repeats the first pick
    _, cnt6, idx6 = bl.select_keypoints_cpu(pc, mask, np.array([1000, 9, 0], np.int32), 16, want_index=True)
    assert cnt6.tolist() == [16, 9, 0] and len(set(idx6[1, :9])) == 9 and (idx6[1, 9:] == idx6[1, 0]).all()
    # a uniform subset: over many frame ids every keypoint of frame 0 is picked about 16 / 40 of the time
    hits = np.zeros(1000)
    for fid in range(400):
        hits[bl.select_keypoints_cpu(pc[:1], mask[:1], None, 16, seed=1, frame_ids=[fid], want_index=True)[2][0]] += 1
    share = hits[mask[0] > 0] / 400
    assert hits[mask[0] == 0].sum() == 0 and abs(share.mean() - 0.4) < 1e-12 and np.abs(share - 0.4).max() < 0.12


def test_random_keypoints():
    pc, _, count = selection_case()
    kp, cnt, idx = bl.random_keypoints_cpu(pc, count, 64, seed=2, frame_ids=[0, 1, 2], want_index=True)
    assert cnt.tolist() == [64, 64, 64]
    for b in range(3):
        assert len(set(idx[b])) == 64 and (idx[b] >= 0).all() and (idx[b] < count[b]).all()
        assert np.array_equal(kp[b], pc[b][:, idx[b]])
    again = bl.random_keypoints_cpu(pc, count, 64, seed=2, frame_ids=[0, 1, 2], want_index=True)[2]
    other = bl.random_keypoints_cpu(pc, count, 64, seed=2, frame_ids=[3, 4, 5], want_index=True)[2]
    assert np.array_equal(again, idx) and not np.array_equal(other, idx)
