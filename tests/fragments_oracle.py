"""numpy float64 restatement of the reference's indoor evaluation, written from reading it
(evaluation/matlab/eval_indoor/3dmatch/register2Fragments.m, writeLog.m, external/ElasticReconstruction/
mrEvaluateRegistrationMy.m with its mrComputeTransformationError and dcm2quat), plus the fixtures the CPU and GPU tests of
f-9 share.  Independent of the product: distances by broadcasting, the union by numpy.unique, the information matrix by the
MATLAB loop, the overlap by all pairs.  RANSAC itself is eval_oracle's (ransacfit / replay / trial)."""
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
