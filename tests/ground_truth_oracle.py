"""getGtInfoLog.m (evaluation/matlab/eval_indoor/3dmatch) restated line by line in float64 numpy, for the f-18 tests: all-pairs
distances in chunks (no tree, no pruning), the moved points by the plain R @ b + t, covMat by the explicit G of the script.
The random thinning is the one thing that cannot be restated (MATLAB's stream): the selection takes the library's keys.

The restated moved points round differently from the library's (another order of the three products), so a row whose restated
distance lies within TOL of a radius may fall on either side: `ambiguous` names those rows and the tests assert how many there
are (none, in every fixture)."""
import functools

import numpy as np

TOL = 1e-9      # metres, absolute


def moved(b, Rt):
    """fragment2Points = relExt(1:3,1:3) * fragment2Points + repmat(relExt(1:3,4), ...)"""
    Rt = np.asarray(Rt, np.float64)
    return (Rt[:3, :3] @ np.asarray(b, np.float64)[:, :3].T + Rt[:3, 3:4]).T


def nearest_distance(a, q, chunk: int = 512):
    """nnDist = sqrt(nnSqrDist) of multiQueryKNNSearchImpl(fragment1, q, 1): for every row of q the distance to the nearest
    row of a, by all pairs; inf when a is empty."""
    a, q = np.asarray(a, np.float64)[:, :3], np.asarray(q, np.float64)
    out = np.full(len(q), np.inf)
    if not len(a):
        return out
    for lo in range(0, len(q), chunk):
        d2 = np.zeros((len(q[lo:lo + chunk]), len(a)))
        for c in range(3):
            d = q[lo:lo + chunk, c:c + 1] - a[None, :, c]
            d2 += d * d
        out[lo:lo + chunk] = np.sqrt(d2.min(1))
    return out


def classes(d, far, near):
    return np.where(d < near, 2, np.where(d < far, 1, 0)).astype(np.uint8)


def ambiguous(d, far, near, tol: float = TOL):
    return (np.abs(d - far) <= tol) | (np.abs(d - near) <= tol)


def reach(a, b, Rt, far=0.03, near=0.006):
    """One pair: a = fragment 1's rows, b = fragment 2's.  -> dict(q, d, cls, hits (far, near), ratio (over n1, over n2),
    ambiguous)"""
    q = moved(b, Rt) if len(b) else np.zeros((0, 3))
    d = nearest_distance(a, q)
    cls = classes(d, far, near)
    n_far = int((d < far).sum())                                      # sum(nnDist < voxelGridSize*5)
    ratio = (n_far / len(a) if len(a) else 0.0, n_far / len(b) if len(b) else 0.0)
    return dict(q=q, d=d, cls=cls, hits=(n_far, int((d < near).sum())), ratio=ratio, ambiguous=ambiguous(d, far, near))


def select(cls, key, cap):
    """The rows of corresQ: every class-2 row, or the `cap` smallest (key, row) of them when there are more -- in that order
    either way (the order the library sums in)."""
    rows = np.nonzero(np.asarray(cls) == 2)[0]
    k = np.asarray(key, np.uint64)[rows]
    return rows[np.lexsort((rows, k))][:int(cap)]


def moved_rounding(b, Rt):
    """What a coordinate of a moved point can differ by between two orders of (r0 b0 + r1 b1 + r2 b2) + t: each order makes
    three roundings on partial sums no larger than |R| |b| + |t|, so 4 ulps of that magnitude cover the pair of them."""
    Rt, b = np.asarray(Rt, np.float64), np.asarray(b, np.float64)[:, :3]
    return 2.0 ** -51 * float((np.abs(Rt[:3, :3]) @ np.abs(b).T + np.abs(Rt[:3, 3:4])).max()) if len(b) else 0.0


def cov_mat(q, dq: float = 0.0):
    """covMat = sum of G'G, G = [eye(3), -Qx], with the per-entry summation-order bound n 2^-52 sum |terms|.  dq > 0 adds what
    an error of dq in every coordinate of q can move an entry by: sum (|G|'dG + dG'|G| + dG'dG), dG = dq where G holds a
    coordinate.  The seeded scenes are compared at dq = 0, the bound of the summation order alone; the constructed cases have
    pairs with one or a handful of near rows, where the order of the sum is no cover for the moved point's own rounding."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    n = len(q)
    Qx = np.zeros((n, 3, 3))
    Qx[:, 0, 1], Qx[:, 0, 2] = -q[:, 2], q[:, 1]
    Qx[:, 1, 0], Qx[:, 1, 2] = q[:, 2], -q[:, 0]
    Qx[:, 2, 0], Qx[:, 2, 1] = -q[:, 1], q[:, 0]
    G = np.concatenate((np.broadcast_to(np.eye(3), (n, 3, 3)), -Qx), 2)
    terms = np.einsum("nki,nkj->nij", G, G)                           # G'*G per row
    bound = n * 2.0 ** -52 * np.abs(terms).sum(0)
    if dq > 0.0:
        dG = np.broadcast_to(np.concatenate((np.zeros((3, 3)), dq * (1.0 - np.eye(3))), 1), (n, 3, 6))
        aG = np.abs(G)
        bound = bound + (np.einsum("nki,nkj->ij", aG, dG) + np.einsum("nki,nkj->ij", dG, aG) + np.einsum("nki,nkj->ij", dG, dG))
    return terms.sum(0), bound


def pair_truth(a, b, Rt, key, cap=5000, far=0.03, near=0.006, with_moved_rounding=False):
    r = reach(a, b, Rt, far, near)
    rows = select(r["cls"], key, cap)
    r["rows"] = rows
    r["info"], r["info_bound"] = cov_mat(r["q"][rows], moved_rounding(b, Rt) if with_moved_rounding else 0.0)
    return r


def fragment_rows(bank, f):
    return np.asarray(bank.rows)[int(bank.offsets[f]):int(bank.offsets[f + 1]), :3]


@functools.lru_cache(maxsize=None)
def seeded_scene(seed=0, fragments=6, points=4000, dim=32):
    from usip_amd import fragments as fr
    return fr.synthetic_scene(seed, fragments, points, dim)


# ------------------------------------------------------------------------------------------------ constructed cases
def rigid(rng, max_angle=1.0, max_shift=0.5, min_angle=0.2):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(min_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    T[:3, 3] = rng.uniform(-max_shift, max_shift, size=3)
    return T


def into_own_frame(world, T):
    """world rows -> the float32 rows of a fragment whose pose (fragment -> world) is T"""
    inv = np.linalg.inv(T)
    return np.ascontiguousarray((np.asarray(world, np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))


def lattice(rng):
    """343 rows inside |x| < 4: a unit grid jittered by 0.2, so any two rows are at least 0.6 m apart"""
    g = np.stack(np.meshgrid(*[np.arange(-3.0, 3.5, 1.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g + rng.uniform(-0.2, 0.2, size=g.shape)).astype(np.float32)


def displaced(rng, rows, dist):
    u = rng.normal(size=(len(rows), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.asarray(rows, np.float64) + np.asarray(dist, np.float64).reshape(-1, 1) * u


def unrelated(rng, n):
    """rows at least 1 m from every lattice row (the lattice ends at |y| <= 3.2), still inside 8 m after any pose of rigid()"""
    return np.stack((rng.uniform(-3, 3, n), rng.uniform(4.5, 5.0, n), rng.uniform(-3, 3, n)), 1)


THRESHOLD_STEPS = ((0.0059, 2), (0.0061, 1), (0.0299, 1), (0.0301, 0))


@functools.lru_cache(maxsize=None)
def constructed_case():
    """One bank: fragment 0 the lattice; fragment 1 the threshold fragment (every lattice row displaced by exactly 0.0059,
    0.0061, 0.0299 or 0.0301 m in turn, plus 40 unrelated rows, shuffled); fragments 2 .. 5 the selection fragments with 6, 7,
    8 and 300 rows displaced by 0.003 m (near), 20 by 0.02 m (far only) and 10 unrelated.  Every fragment 2 lives in its own
    frame; the test's Rt is that pose.  float32 rounding below 8 m is <= 4.8e-7 per axis, the margins are 1e-4."""
    rng = np.random.default_rng(1806)
    a = lattice(rng)
    clouds, Rt, expect = [a], [], []
    steps = np.array([THRESHOLD_STEPS[i % 4][0] for i in range(len(a))])
    want = np.array([THRESHOLD_STEPS[i % 4][1] for i in range(len(a))] + [0] * 40, np.uint8)
    world = np.concatenate((displaced(rng, a, steps), unrelated(rng, 40)))
    shuffle = rng.permutation(len(world))
    T = rigid(rng)
    clouds.append(into_own_frame(world[shuffle], T))
    Rt.append(T[:3])
    expect.append(want[shuffle])
    for k in (6, 7, 8, 300):
        near_rows = rng.choice(len(a), k, replace=False)
        rest = np.setdiff1d(np.arange(len(a)), near_rows)[:20]
        world = np.concatenate((displaced(rng, a[near_rows], np.full(k, 0.003)), displaced(rng, a[rest], np.full(20, 0.02)),
                                unrelated(rng, 10)))
        want = np.array([2] * k + [1] * 20 + [0] * 10, np.uint8)
        shuffle = rng.permutation(len(world))
        T = rigid(rng)
        clouds.append(into_own_frame(world[shuffle], T))
        Rt.append(T[:3])
        expect.append(want[shuffle])
    return dict(clouds=clouds, frag1=np.zeros(5, np.int32), frag2=np.arange(1, 6, dtype=np.int32), Rt=np.stack(Rt),
                expect=expect, near_counts=(len(a) // 4 + (len(a) % 4 > 0), 6, 7, 8, 300))


EDGE_N1, EDGE_N2 = (1, 255, 256, 257, 513), (1, 256, 257, 600)


@functools.lru_cache(maxsize=None)
def tile_edge_case():
    """One bank and one batch of mixed lengths around the 256-row tile and workgroup; the longest fragment has 600 rows, so
    lmax is no multiple of 64.  Rows are uniform in a beam 1 m long along x and 0.05 m across, so a fair share of every
    fragment lies within either radius and the walk has tiles to skip.
    Fragments: 0 .. 4 the n1 lengths, 5 .. 8 the n2 lengths, 9 empty, 10 all rows at one x (the walk cannot prune), 11 a box
    12 m away (the walk ends in its first round), 12 a fragment whose rows each appear twice, 13 a copy of it.
    -> dict(clouds, frag1, frag2, Rt, mask)"""
    rng = np.random.default_rng(256)
    box = lambda n: (rng.uniform(0.0, 1.0, size=(n, 3)) * (1.0, 0.05, 0.05)).astype(np.float32)       # noqa: E731
    clouds = [box(n) for n in EDGE_N1 + EDGE_N2] + [np.zeros((0, 3), np.float32)]
    same_x = box(300)
    same_x[:, 0] = 0.5
    away = box(300) + np.float32(12.0)
    twice = np.concatenate((box(150),) * 2)
    clouds += [same_x, away, twice, twice.copy()]
    pairs = [(i, 5 + j) for i in range(5) for j in range(4)]
    pairs += [(9, 8), (4, 9), (3, 7), (10, 8), (4, 11), (11, 4), (12, 13), (8, 10)]
    mask = np.ones(len(pairs), np.uint8)
    mask[22] = 0                                                               # (3, 7) again, masked
    Rt = np.stack([rigid(rng, 0.02, 0.01, 0.0)[:3] for _ in pairs])
    Rt[25], Rt[26] = np.eye(4)[:3], np.eye(4)[:3]                              # the far box stays far; duplicates coincide
    return dict(clouds=clouds, frag1=np.array([p[0] for p in pairs], np.int32), frag2=np.array([p[1] for p in pairs], np.int32),
                Rt=Rt, mask=mask, zero_pairs=(20, 21, 22))


def check_pairs_against_restatement(bank, frag1, frag2, Rt, out, info=None, cap=5000, mask=None, far=0.03, near=0.006,
                                    with_moved_rounding=False):
    """Every pair of a batch against pair_truth: cls over the unambiguous rows, hits exactly, info within the summation bound.
    -> the number of rows left out (the caller asserts it)."""
    left_out = 0
    for p in range(len(frag2)):
        a, b = fragment_rows(bank, frag1[p]), fragment_rows(bank, frag2[p])
        if mask is not None and not mask[p]:
            a = a[:0]
        r = pair_truth(a, b, Rt[p], np.asarray(out["key"][p, :len(b)]).astype(np.uint64), cap, far, near,
                       with_moved_rounding)
        keep = ~r["ambiguous"]
        left_out += int(r["ambiguous"].sum())
        assert np.array_equal(np.asarray(out["cls"][p, :len(b)])[keep], r["cls"][keep]), p
        assert not np.asarray(out["cls"][p, len(b):]).any(), p
        if not r["ambiguous"].any():
            assert tuple(int(v) for v in out["hits"][p]) == r["hits"], (p, out["hits"][p], r["hits"])
            if mask is None or mask[p]:
                assert tuple(float(v) for v in out["ratio"][p]) == r["ratio"], (p, out["ratio"][p], r["ratio"])
            if info is not None:
                err = np.abs(np.asarray(info[p]) - r["info"])
                assert (err <= r["info_bound"]).all(), (p, err.max(), r["info_bound"].max())
    return left_out
