"""numpy float64 restatement of the reference's MATLAB evaluation, written from reading it
(evaluation/matlab/eval_outdoor/external/estimateRigidTransform.m, quat2rot.m, ransacfitRt.m, ransac.m,
eval_outdoor/Utils.m compareTransform, eval_repeatability/eval_rep.m, evaluate_kitti.m's pdist2 matching).

Independent of the product's solver: the eigenvector comes from numpy.linalg.eigh, not from a Jacobi iteration.
Shapes follow the product's batches: x1, x2 are [3, n] (x1 = R x2 + t)."""
import numpy as np

EPS = np.finfo(np.float64).eps


def quat2rot(q):
    q0, q1, q2, q3 = q
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def cross_matrix(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def estimate_rigid_transform(x, y):
    """x, y float [3, n] -> (Rt [3, 4] with x = R y + t, eigenvalues ascending)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[1]
    xc, yc = x.sum(1) / n, y.sum(1) / n
    xs, ys = x - xc[:, None], y - yc[:, None]
    B = np.zeros((4, 4))
    for i in range(n):
        A = np.zeros((4, 4))
        A[0, 1:] = ys[:, i] - xs[:, i]
        A[1:, 0] = xs[:, i] - ys[:, i]
        A[1:, 1:] = cross_matrix(ys[:, i] + xs[:, i])
        B += A.T @ A
    w, v = np.linalg.eigh(B)
    R = quat2rot(v[:, 0])
    return np.concatenate((R, (xc - R @ yc)[:, None]), 1), w


def residuals(Rt, x1, x2):
    d = np.asarray(x1, np.float64) - (Rt[:, :3] @ np.asarray(x2, np.float64) + Rt[:, 3:4])
    return np.sqrt((d ** 2).sum(0))


def trial(x1, x2, triplet, threshold):
    """-> (Rt, inlier count, eigen-gap ratio (l1 - l0) / lmax, distance of the closest residual to the threshold)."""
    t = np.asarray(triplet)
    Rt, w = estimate_rigid_transform(x1[:, t], x2[:, t])
    d = residuals(Rt, x1, x2)
    gap = (w[1] - w[0]) / w[3] if w[3] > 0 else 0.0
    return Rt, int((d < threshold).sum()), gap, float(np.abs(d - threshold).min())


def trials_needed(best, npts):
    f = best / npts
    p_no = min(1 - EPS, max(EPS, 1 - f ** 3))
    return max(np.log(1 - 0.99) / np.log(p_no), 10)


def replay(counts, npts, max_trials):
    """ransac.m's loop over given scores -> (chosen trial, trialcount)."""
    best, N, trialcount, chosen = 0, 1, 0, 0
    while N > trialcount:
        if counts[trialcount] >= best:
            best, chosen = counts[trialcount], trialcount
            N = trials_needed(best, npts)
        trialcount += 1
        if trialcount > max_trials:
            break
    return chosen, trialcount


def rotm2eul_zyx(R):
    sy = np.hypot(R[0, 0], R[1, 0])
    if sy < 10 * EPS:
        return np.array([0.0, np.arctan2(-R[2, 0], sy), np.arctan2(-R[1, 2], R[1, 1])])
    return np.array([np.arctan2(R[1, 0], R[0, 0]), np.arctan2(-R[2, 0], sy), np.arctan2(R[2, 1], R[2, 2])])


def compare_transform(A, B):
    delta_t = np.linalg.norm(A[:, 3] - B[:, 3])
    return delta_t, np.abs(rotm2eul_zyx(A[:, :3].T @ B[:, :3])).sum() * 180 / np.pi


def ransacfit(x1, x2, threshold, max_trials, triplets, gt=None):
    """ransacfitRt on a given triplet sequence ([T, 3]) -> dict(valid, Rt, inliers (indices), trialcount, chosen,
    delta_t, delta_deg)."""
    n = x1.shape[1]
    out = dict(valid=False, Rt=None, inliers=np.zeros(0, int), trialcount=0, chosen=0, delta_t=3.0, delta_deg=6.0)
    if n < 3:
        return out
    if n == 3:
        out.update(valid=True, Rt=estimate_rigid_transform(x1, x2)[0], inliers=np.arange(3))
    else:
        best, N, trialcount, chosen, best_in = 0, 1, 0, 0, None
        while N > trialcount:
            t = np.asarray(triplets[trialcount])
            Rt, _ = estimate_rigid_transform(x1[:, t], x2[:, t])
            inl = np.nonzero(residuals(Rt, x1, x2) < threshold)[0]
            if len(inl) >= best:
                best, chosen, best_in = len(inl), trialcount, inl
                N = trials_needed(best, n)
            trialcount += 1
            if trialcount > max_trials:
                break
        out.update(trialcount=trialcount, chosen=chosen)
        if len(best_in) >= 3:
            out.update(valid=True, Rt=estimate_rigid_transform(x1[:, best_in], x2[:, best_in])[0], inliers=best_in)
    if gt is not None and out["valid"]:
        out["delta_t"], out["delta_deg"] = compare_transform(np.asarray(gt, np.float64), out["Rt"])
    return out


def repeatability(anc, pos, gt, radius):
    """anc [3, na], pos [3, np] -> (min distances [na], hits, ratio)."""
    q = gt[:, :3] @ np.asarray(pos, np.float64) + gt[:, 3:4]
    d = np.sqrt(((np.asarray(anc, np.float64)[:, :, None] - q[:, None, :]) ** 2).sum(0))
    m = d.min(1) if q.shape[1] else np.full(anc.shape[1], np.inf)
    hits = int((m < radius).sum())
    return m, hits, hits / anc.shape[1] if anc.shape[1] else 0.0


def match(anc_desc, pos_desc):
    """anc_desc [C, na], pos_desc [C, np] -> (first arg-min [na], sorted two smallest distances [na, 2])."""
    a, b = np.asarray(anc_desc, np.float64), np.asarray(pos_desc, np.float64)
    d = np.concatenate([np.sqrt(((a.T[i:i + 32, None, :] - b.T[None, :, :]) ** 2).sum(2))
                        for i in range(0, a.shape[1], 32)]) if a.shape[1] else np.zeros((0, b.shape[1]))
    two = np.sort(d, 1)[:, :2] if b.shape[1] > 1 else np.concatenate((d, np.full_like(d, np.inf)), 1)
    return d.argmin(1), two


# ------------------------------------------------------------------ the issue's generator
def random_rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = cross_matrix(axis)
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_pair(rng, n=512, inlier_share=0.4, noise=0.15):
    """-> (x1 f32 [3, n], x2 f32 [3, n], gt [3, 4]): y uniform in +-40 x +-40 x +-4 m, x = R y + t + N(0, noise), the
    rest of the rows of x replaced by uniform outliers."""
    lo, hi = np.array([-40.0, -40.0, -4.0]), np.array([40.0, 40.0, 4.0])
    y = rng.uniform(lo, hi, size=(n, 3))
    R = random_rotation(rng, 0.3 * rng.uniform(0.8, 1.2))
    t = rng.uniform(-4, 4, size=3)
    x = y @ R.T + t + rng.normal(0, noise, size=(n, 3))
    out = rng.permutation(n)[: int(round(n * (1 - inlier_share)))]
    x[out] = rng.uniform(lo, hi, size=(len(out), 3))
    return (np.ascontiguousarray(x.T, np.float32), np.ascontiguousarray(y.T, np.float32),
            np.concatenate((R, t[:, None]), 1))


def make_batch(seed, P=4, n=512, T=2000, nmax=None, counts=None, **kw):
    """-> x1, x2 f32 [P, 3, nmax], count i32 [P], gt f64 [P, 3, 4], triplets i32 [P, T, 3]."""
    rng = np.random.default_rng(seed)
    nmax = nmax or n
    counts = [n] * P if counts is None else counts
    x1, x2 = np.zeros((P, 3, nmax), np.float32), np.zeros((P, 3, nmax), np.float32)
    gt, tri = np.zeros((P, 3, 4)), np.zeros((P, T, 3), np.int32)
    for p in range(P):
        c = counts[p]
        if c > 0:
            a, b, g = make_pair(rng, c, **kw)
            x1[p, :, :c], x2[p, :, :c], gt[p] = a, b, g
        if c >= 3:
            tri[p] = np.stack([rng.choice(c, 3, replace=False) for _ in range(T)])
    return x1, x2, np.asarray(counts, np.int32), gt, tri
