"""numpy float64 restatement of the reference's indoor evaluation, written from reading it
(evaluation/matlab/eval_indoor/3dmatch/register2Fragments.m, writeLog.m, external/ElasticReconstruction/
mrEvaluateRegistrationMy.m with its mrComputeTransformationError and dcm2quat), plus the fixtures the CPU and GPU tests of
f-9 share.  Independent of the product: distances by broadcasting, the union by numpy.unique, the information matrix by the
MATLAB loop, the overlap by all pairs.  RANSAC itself is eval_oracle's (ransacfit / replay / trial)."""
import functools

import numpy as np

import eval_oracle as eo

REL_GAP = 1e-5          # eval_oracle.match's float32 bound: two distances closer than this, relatively, may swap in float32


def topk(a_desc, b_desc, k):
    """a_desc [C, na], b_desc [C, nb] -> (idx [na, min(k, nb)] ascending with ties to the lower index, clear [na]: every gap
    between consecutive ranks 1 .. k + 1 exceeds REL_GAP of the larger distance)."""
    a, b = np.asarray(a_desc, np.float64), np.asarray(b_desc, np.float64)
    na, nb = a.shape[1], b.shape[1]
    kk = min(k, nb)
    if na == 0 or nb == 0:
        return np.zeros((na, kk), int), np.ones(na, bool)
    d = np.concatenate([np.sqrt(((a.T[i:i + 32, None, :] - b.T[None, :, :]) ** 2).sum(2)) for i in range(0, na, 32)])
    order = np.argsort(d, 1, kind="stable")
    ranked = np.take_along_axis(d, order, 1)[:, :min(k + 1, nb)]
    gaps = ranked[:, 1:] - ranked[:, :-1]
    clear = (gaps >= REL_GAP * ranked[:, 1:]).all(1) if ranked.shape[1] > 1 else np.ones(na, bool)
    return order[:, :kk], clear


def union(nn12, nn21):
    """nn12 [na, k12] (indices into fragment 2), nn21 [nb, k21] (into fragment 1) -> union(..., 'rows'), 0-based."""
    na, nb = nn12.shape[0], nn21.shape[0]
    m12 = np.stack((np.repeat(np.arange(na), nn12.shape[1]), nn12.reshape(-1)), 1)
    m21 = np.stack((nn21.reshape(-1), np.repeat(np.arange(nb), nn21.shape[1])), 1)
    both = np.concatenate((m12, m21)).astype(np.int64)
    return np.unique(both, axis=0) if len(both) else both.reshape(0, 2)


def information(points):
    """register2Fragments.m:78-87 as written -> (matrix [6, 6], the sum of the terms' magnitudes [6, 6])."""
    info, mag = np.zeros((6, 6)), np.zeros((6, 6))
    for sx, sy, sz in np.asarray(points, np.float64).reshape(-1, 3):
        A = np.array([[1, 0, 0, 0, 2 * sz, -2 * sy], [0, 1, 0, -2 * sz, 0, 2 * sx], [0, 0, 1, 2 * sy, -2 * sx, 0]])
        info += A.T @ A
        mag += np.abs(A).T @ np.abs(A)
    return info, mag


def nearest_distance(a, b):
    """a [na, 3], b [nb, 3] float64 -> for every row of a the distance to its nearest row of b (all pairs)."""
    out = np.full(len(a), np.inf)
    if len(b):
        for i in range(0, len(a), 256):
            out[i:i + 256] = np.sqrt(((a[i:i + 256, None, :] - b[None, :, :]) ** 2).sum(2)).min(1)
    return out


def overlap(a, b, Rt, radius):
    """ratioAligned: a, b float32 [n, 3], Rt [3, 4] -> (hits (2,), ratio (2,), points within 1e-9 of the radius)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64) @ Rt[:, :3].T + Rt[:, 3]
    d1, d2 = nearest_distance(a, b), nearest_distance(b, a)
    hits = np.array([(d1 < radius).sum(), (d2 < radius).sum()])
    near = int((np.abs(d1 - radius) < 1e-9).sum() + (np.abs(d2 - radius) < 1e-9).sum())
    ratio = np.array([hits[0] / len(a) if len(a) else 0.0, hits[1] / len(b) if len(b) else 0.0])
    return hits, ratio, near


def dcm2quat(D):
    q0 = 0.5 * np.sqrt(1 + D[0, 0] + D[1, 1] + D[2, 2])
    return np.array([q0, -(D[2, 1] - D[1, 2]) / (4 * q0), -(D[0, 2] - D[2, 0]) / (4 * q0), -(D[1, 0] - D[0, 1]) / (4 * q0)])


def transformation_error(gt_trans, result_trans, info):
    trans = np.linalg.solve(gt_trans, result_trans)
    with np.errstate(all="ignore"):
        er = np.concatenate((trans[:3, 3], -dcm2quat(trans[:3, :3])[1:]))
        return er @ info @ er / info[0, 0]


# ------------------------------------------------------------------ fixtures shared by the CPU and the GPU tests
def unit_descriptors(rng, B, C, M):
    d = rng.normal(size=(B, C, M))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def topk_fixture():
    """Random unit descriptors, D = 128: (anc [B, C, Ma], pos [B, C, Nb], na, nb) with ragged counts, among them
    databases of 0, 1 and k - 1 rows for k = 5 and 8."""
    rng = np.random.default_rng(TOPK_SEED)
    anc, pos = unit_descriptors(rng, 6, 128, 48), unit_descriptors(rng, 6, 128, 160)
    na = np.array([48, 48, 7, 48, 48, 0], np.int32)
    nb = np.array([160, 0, 1, 4, 7, 160], np.int32)
    return anc, pos, na, nb


TOPK_SEED = 9           # chosen so that the oracle alone leaves out no row at k = 1, 5, 8 (the tests assert it)


def ransac_fixture(n, T, seed):
    """One pair of n correspondences (40 % inliers at 0.05 m noise, as fragments' keypoints are) with T explicit triplets."""
    return eo.make_batch(seed, P=1, n=n, T=T, noise=0.05)


def room_pair(seed, n=5000):
    """Two overlapping fragments of a box room's surfaces, about n points each, in their own frames, and the pose moving
    the second into the first's frame (with a small error, as an estimate has)."""
    rng = np.random.default_rng(seed)

    def surface(m, lo, hi):
        p = rng.uniform(size=(m, 3)) * np.array([hi - lo, 3.0, 2.5]) + np.array([lo, 0, 0])
        face = rng.integers(0, 4, size=m)
        p[face == 0, 2] = 0.0
        p[face == 1, 2] = 2.5
        p[face == 2, 1] = 0.0
        p[face == 3, 1] = 3.0
        return p
    a_world, b_world = surface(n, 0.0, 4.0), surface(n, 2.0, 6.0)
    R = eo.random_rotation(rng, 0.7)
    t = rng.uniform(-1, 1, size=3)
    b_own = (b_world - t) @ R                                          # b_world = R b_own + t
    Rt = np.concatenate((eo.random_rotation(rng, 0.01) @ R, (t + rng.normal(0, 0.02, 3))[:, None]), 1)
    return a_world.astype(np.float32), b_own.astype(np.float32), Rt


def awkward_topk_fixture():
    """Shapes top-k kernels go wrong at: C = 33, Ma = 45 (no multiple of the four rows a workgroup takes), databases of 515,
    257, 256 and 255 rows (around one pass of a wave, 64 * 4 candidates) and a single query row.  The oracle alone leaves
    out no row at any k in 1 .. 8, which is asserted here, so that every row binds."""
    rng = np.random.default_rng(AWKWARD_SEED)
    anc, pos = unit_descriptors(rng, 4, 33, 45), unit_descriptors(rng, 4, 33, 515)
    na, nb = np.array([45, 43, 1, 42], np.int32), np.array([515, 257, 256, 255], np.int32)
    for k in range(1, 9):
        for p in range(len(na)):
            assert topk(anc[p][:, :na[p]], pos[p][:, :nb[p]], k)[1].all(), (k, p)
    return anc, pos, na, nb


AWKWARD_SEED = 100      # the oracle leaves out 0 of 131 rows for every k (seed 102 leaves out 2 at k = 5)

# ---- an exact lattice for the overlap: every coordinate an integer times H, the pose a quarter turn and an integer shift
H = 1.0 / 64
LATTICE_RADIUS = 20 * H                                                  # 0.3125: squared, 400 H^2
QUARTER_TURN = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
# partners at exactly the radius (|o|^2 = 400) and just inside it (398, 393, 398)
LATTICE_OFFSETS = np.array([(20, 0, 0), (-20, 0, 0), (0, 12, 16), (0, 12, -16), (0, -12, 16), (0, -12, -16), (12, 16, 0),
                            (-16, 0, 12), (0, 0, 20), (19, 6, 1), (11, 16, 4), (13, 15, 2)], np.int64)
LATTICE_SIZES = {"small": (4000, 3500, 400, 1500, 7), "large": (30000, 23000, 800, 8000, 8)}   # n1, n2, span, planted, seed


def nearest_sq_int(a, b):
    """a [na, 3], b [nb, 3] int64 with |coordinates| < 2^20 -> for every row of a the smallest squared distance to a row of
    b, an exact integer: |a|^2 + |b|^2 - 2 a.b with the products taken by the float64 matrix product, whose operands and
    partial sums are integers below 2^43, so nothing rounds."""
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)) < 2 ** 20
    af, bf = a.astype(np.float64), b.astype(np.float64)
    a2, b2 = (af * af).sum(1), (bf * bf).sum(1)
    out = np.zeros(len(a), np.int64)
    for i in range(0, len(a), 1024):
        d2 = (a2[i:i + 1024, None] + b2[None, :]) - 2.0 * (af[i:i + 1024] @ bf.T)
        out[i:i + 1024] = d2.min(1).astype(np.int64)
    return out


def inverse_pose(Rt):
    return np.concatenate((Rt[:, :3].T, -(Rt[:, :3].T @ Rt[:, 3:4])), 1)


@functools.lru_cache(maxsize=None)
def lattice_pair(size):
    """-> (a f32 [n1, 3], b f32 [n2, 3] in its own frame, Rt f64 [3, 4] moving b into a's frame, hits (2,) by integer
    arithmetic, queries decided by equality alone (2,)).  Coordinates are integers times H = 1 / 64, exact in float32; under
    the quarter turn and the integer shift every moved coordinate, every squared distance and sqrt(400 H^2) = 20 H are
    exact in float64, so a query hits iff some point of the other fragment has squared integer distance < 400.  Fragment 2
    holds planted partners of a random subset of fragment 1, many of them at exactly the radius, plus random points.
    Asserted here: in either direction at least 100 queries have their nearest point at exactly the radius (a `<=`, a
    dropped square root or a guard cutting early moves the count by that many) and the hit share is inside (0.5, 0.95)."""
    n1, n2, span, planted, seed = LATTICE_SIZES[size]
    rng = np.random.default_rng(seed)
    ai = rng.integers(0, span, size=(n1, 3))
    src = rng.choice(n1, planted, replace=False)
    bi = np.concatenate((ai[src] + LATTICE_OFFSETS[rng.integers(0, len(LATTICE_OFFSETS), planted)],
                         rng.integers(0, span, size=(n2 - planted, 3))))
    bi = bi[rng.permutation(n2)]
    shift = np.array([37, -150, 64], np.int64)
    R = QUARTER_TURN.astype(np.int64)
    own = (bi - shift) @ R                                               # bi = R own + shift
    assert np.array_equal(own @ R.T + shift, bi)
    a, b = (ai * H).astype(np.float32), (own * H).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), ai * H) and np.array_equal(b.astype(np.float64), own * H)
    Rt = np.concatenate((QUARTER_TURN, (shift * H)[:, None]), 1)
    assert np.array_equal(b.astype(np.float64) @ Rt[:, :3].T + Rt[:, 3], bi * H)
    d12, d21 = nearest_sq_int(ai, bi), nearest_sq_int(bi, ai)
    hits = np.array([(d12 < 400).sum(), (d21 < 400).sum()])
    equal = np.array([(d12 == 400).sum(), (d21 == 400).sum()])
    assert (equal >= 100).all(), equal
    assert 0.5 < hits[0] / n1 < 0.95 and 0.5 < hits[1] / n2 < 0.95, hits
    assert np.sqrt(400 * H * H) == LATTICE_RADIUS
    return a, b, Rt, hits, equal


# ---- constant-x walls at the benchmark's size
WALL_RADIUS = 0.2
WALL_POSE = np.concatenate((QUARTER_TURN, np.array([[1.0], [-2.0], [0.5]])), 1)


def box_room(rng, n, origin):
    """n points on the six faces of a 4 x 3 x 2.5 m box at `origin`, a face per point with equal chance."""
    p = rng.uniform(size=(n, 3)) * np.array([4.0, 3.0, 2.5])
    face = rng.integers(0, 6, size=n)
    for f, (axis, value) in enumerate(((0, 0.0), (0, 4.0), (1, 0.0), (1, 3.0), (2, 0.0), (2, 2.5))):
        p[face == f, axis] = value
    return p + np.asarray(origin)


def longest_run(v):
    """The longest run of equal values in sorted(v)."""
    s = np.sort(np.asarray(v).ravel())
    edges = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1], [True])))
    return int(np.diff(edges).max()) if len(s) else 0


def tree_overlap(a, b, Rt, radius):
    """overlap() with scipy's k-d tree on float64 in place of all pairs: for fragments of 100 000 points."""
    from scipy.spatial import cKDTree
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64) @ Rt[:, :3].T + Rt[:, 3]
    if not len(a) or not len(b):
        return np.zeros(2, int), np.zeros(2), 0
    d1, d2 = cKDTree(b).query(a)[0], cKDTree(a).query(b)[0]
    hits = np.array([(d1 < radius).sum(), (d2 < radius).sum()])
    near = int((np.abs(d1 - radius) < 1e-9).sum() + (np.abs(d2 - radius) < 1e-9).sum())
    return hits, hits / np.array([len(a), len(b)]), near


@functools.lru_cache(maxsize=None)
def wall_rooms(n=100000):
    """-> (clouds [room 1, room 2 in its own frame, 300 points of room 1, no points, 512 points of room 1], Rt, hits (2,)
    of the pair (room 1, room 2) by the k-d tree).  Two box rooms of n points with points on all six faces, the second
    2.0 m along x and 0.5 m along y from the first and stored under the exact quarter turn, so that the static x of
    room 1 and the MOVED x of room 2 both have runs of about n / 6 equal values (65 tiles of the overlap walk at
    n = 100 000).  Asserted here: no distance within 1e-9 of the radius, a hit share inside (0.1, 0.9) in either
    direction, a longest run of equal x of at least n / 10 in both fragments."""
    rng = np.random.default_rng(61)
    a = box_room(rng, n, (0.0, 0.0, 0.0)).astype(np.float32)
    world = box_room(rng, n, (2.0, 0.5, 0.0))
    b = ((world - WALL_POSE[:, 3]) @ QUARTER_TURN).astype(np.float32)    # world = R own + t
    moved_x = b.astype(np.float64) @ WALL_POSE[0, :3] + WALL_POSE[0, 3]
    assert longest_run(a[:, 0]) >= n // 10 and longest_run(moved_x) >= n // 10
    hits, ratio, near = tree_overlap(a, b, WALL_POSE, WALL_RADIUS)
    assert near == 0 and (ratio > 0.1).all() and (ratio < 0.9).all(), (hits, near)
    return [a, b, a[:300].copy(), np.zeros((0, 3), np.float32), a[:512].copy()], WALL_POSE, hits


def far_pose(Rt, along_x):
    out = Rt.copy()
    out[0, 3] += along_x
    return out


# ---- the reference's protocol at full size: 1024 keypoints, k = 5, 30 000 trials
FULL_SCENE = dict(seed=3, fragments=3, points=20000, landmarks=1400)
FULL_KEYPOINTS = (1021, 1004, 1020)
FULL_MATCHES = (6175, 6258, 6179)            # the union's rows per pair (0, 1), (0, 2), (1, 2): seven LDS chunks
FULL_TRIALCOUNT = (1987, 4204, 1844)
FULL_SCORE = dict(recall=1.0, precision=1.0, good=1, written=3)


def stack_scene(sc, top, dim=128):
    """The scene's keypoints and descriptors at one width, as FragmentEvaluator.stacked() holds them, and all pairs i < j."""
    F = len(sc["clouds"])
    kp, de, cnt = np.zeros((F, 3, top), np.float32), np.zeros((F, dim, top), np.float32), np.zeros(F, np.int32)
    for i in range(F):
        n = len(sc["xyz"][i])
        kp[i, :, :n], de[i, :, :n], cnt[i] = sc["xyz"][i].T, sc["desc"][i].T, n
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    return kp, de, cnt, np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
