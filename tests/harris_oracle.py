"""An independent restatement of the Harris3D contract (include/usip_hip.h f-16) in numpy float64: an all-pairs
distance matrix, numpy.linalg.eigh, numpy's own summation order.  It shares nothing with the product.

Slab clouds are useless here (one normal direction: det ~ 0); the inputs are noisy box surfaces, whose edges and corners
mix two and three normal directions.

Besides its results it returns three MARGINS, because a comparison with it is meaningful only where no decision sits on a
threshold: `gap` = the smallest relative eigen-gap (l2 - l1) / trace of a point covariance that yields a normal (the
conditioning of the estimated normals), `thr` = the smallest relative distance of a positive response from the threshold,
`tie` = the smallest NONZERO relative response difference between a point at or above the threshold and a member of its
neighbourhood (points with the same member set have bit-equal responses on every side -- identical sums in the same order --
and under the tie rule both stay; they are left out).  A test first asserts all three exceed iss_oracle.MARGIN -- a condition
on its input, not on the product.  `kappa` = the largest ratio of a point's raw second moment sum |d|^2 to m * trace of its
covariance about the mean, and `m_max` the largest member count: what the bound on an estimated normal's error needs."""
import numpy as np

from iss_oracle import MARGIN  # noqa: F401   (1e-9)

RADIUS, THRESHOLD = 1.0, 0.001
# (seed, n, h): n points on the faces of a box of half-sizes (h, 0.6 h, 0.4 h), 0.02 N(0,1) noise, a random rotation.
# Checked on a CPU with this file alone at radius 1, threshold 0.001: gap >= 5.5e-2, thr >= 2.7e-4, tie >= 1.9e-6,
# kappa <= 2.1, 13 to 713 members per query, 223 to 2842 points at or above the threshold, and these keypoint counts (the
# eight of the middle two are the box's corners)
INPUTS = ((0, 257, 2.0), (1, 1000, 3.0), (2, 3000, 5.0), (3, 3000, 1.5))
KEYPOINTS = {(0, 257, 2.0): 4, (1, 1000, 3.0): 8, (2, 3000, 5.0): 8, (3, 3000, 1.5): 2}
METHODS = ("harris", "noble", "lowe", "tomasi")


def _faces(rng, n, h):
    """points f64 [n,3] on the box's faces (a face with probability proportional to its area, uniform on it) and the
    outward unit normal of each point's face f64 [n,3]"""
    half = np.array([h, 0.6 * h, 0.4 * h])
    area = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]])       # of the faces across x, y, z
    axis = rng.choice(3, size=n, p=area / area.sum())
    sign = rng.choice([-1.0, 1.0], size=n)
    p = rng.uniform(-1.0, 1.0, (n, 3)) * half
    p[np.arange(n), axis] = sign * half[axis]
    nrm = np.zeros((n, 3))
    nrm[np.arange(n), axis] = sign
    return p, nrm


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def boxes(seed: int, n: int, h: float, want_normals: bool = False):
    """float32 [3,n]; with want_normals also the rotated analytic face normals float32 [3,n]"""
    rng = np.random.RandomState(seed)
    p, nrm = _faces(rng, n, h)
    p = p + 0.02 * rng.normal(size=(n, 3))
    R = _rotation(rng)
    pc = (p @ R.T).T.astype(np.float32)
    return (pc, (nrm @ R.T).T.astype(np.float32)) if want_normals else pc


def _response(C, method):
    c00, c01, c02, c11, c12, c22 = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    trace = c00 + c11 + c22
    det = c00 * c11 * c22 + 2 * c01 * c02 * c12 - c02 ** 2 * c11 - c01 ** 2 * c22 - c12 ** 2 * c00
    with np.errstate(divide="ignore", invalid="ignore"):
        if method == "harris":
            r = 0.04 + det - 0.04 * trace * trace
        elif method == "noble":
            r = det / trace
        elif method == "lowe":
            r = det / (trace * trace)
        elif method == "tomasi":
            r = np.linalg.eigvalsh(C)[:, 0]
        else:
            raise ValueError(method)
    return np.where((trace == 0) | ~np.isfinite(r), 0.0, r)


def harris(pc, radius=RADIUS, threshold=THRESHOLD, normals=None, response="harris", min_neighbors=3):
    """pc [3,n], normals [3,n] or None -> dict(mask bool [n], response [n], members [n], normals [n,3], neighbours [n] or
    None, gap, thr, tie, kappa, m_max)."""
    p = np.asarray(pc, dtype=np.float64).T                             # [n,3]
    n = len(p)
    d = p[None, :, :] - p[:, None, :]                                  # d[i,j] = p_j - p_i
    d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
    near = d2 < radius * radius
    gap, kappa, neighbours = np.inf, 0.0, None
    if normals is None:
        neighbours = near.sum(1)
        w = near.astype(np.float64)
        mean = np.einsum("ij,ija->ia", w, d) / neighbours[:, None]
        dc = d - mean[:, None, :]
        C = np.einsum("ij,ija,ijb->iab", w, dc, dc) / neighbours[:, None, None]
        lam, vec = np.linalg.eigh(C)                                   # ascending
        nrm = vec[:, :, 0].copy()
        tr = lam.sum(1)
        flat = tr == 0
        nrm[flat] = (0.0, 0.0, 1.0)
        has = neighbours >= min_neighbors
        nrm[~has] = 0.0
        ok = has & ~flat
        if ok.any():
            gap = float(((lam[ok, 1] - lam[ok, 0]) / tr[ok]).min())
            raw = np.einsum("ij,ija,ija->i", w, d, d)
            kappa = float((raw[ok] / (neighbours[ok] * tr[ok])).max())
    else:
        nrm = np.asarray(normals, dtype=np.float32).astype(np.float64).T.copy()
        has = np.isfinite(nrm).all(1) & (nrm != 0).any(1)
        nrm[~has] = 0.0
    w = (near & has[None, :]).astype(np.float64)
    k = w.sum(1)
    C = np.einsum("ij,ja,jb->iab", w, nrm, nrm) / np.maximum(k, 1)[:, None, None]
    res = np.where(has, _response(C, response), 0.0)
    members = np.where(has, k, 0).astype(np.int32)
    kept = np.where(res >= threshold, res, 0.0)
    larger = (near & (kept[None, :] > kept[:, None])).any(1)
    mask = (kept > 0) & ~larger
    pos = res[res > 0]
    thr = float((np.abs(pos - threshold) / threshold).min()) if pos.size and threshold > 0 else np.inf
    pair = near & ~np.eye(n, dtype=bool) & (kept > 0)[:, None]
    si, sj = np.broadcast_to(res[:, None], (n, n))[pair], np.broadcast_to(res[None, :], (n, n))[pair]
    rel = np.abs(si - sj) / np.maximum(np.abs(si), np.abs(sj))
    rel = rel[rel > 0]
    return dict(mask=mask, response=res, members=members, normals=nrm,
                neighbours=None if neighbours is None else neighbours.astype(np.int32), above=int((kept > 0).sum()),
                gap=gap, thr=thr, tie=float(rel.min()) if rel.size else np.inf, kappa=kappa,
                m_max=int(near.sum(1).max()))
