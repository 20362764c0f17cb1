"""An independent numpy restatement of the FPFH baseline descriptor (include/usip_hip.h f-19): all pairs, np.arctan2
for the angle feature, plain np.sum for every sum.  It shares no code with csrc/fpfh_math.h.  Beside its results it reports
the smallest RELATIVE MARGIN of any decision it took, so that a test can first assert that no decision of the frame is within
rounding of its threshold and then ask for equal counts:

  d2 against r * r                      |d2 - r2| / r2
  f4 = |d| against 0                    f4 / r
  |a1| against |a2|                     ||a1| - |a2|| / max(|a1|, |a2|)
  |v| against 0                         |v| / |d|                    (unit normals: the sine of the angle between d and n1)
  f2, f3 against their bin edges        the distance of 11 (f + 1) / 2 to the nearest of the edges 1 .. 10, in bins
  the angle against its bin edges       the distance of 11 (theta + pi) / (2 pi) to the nearest integer, in bins, times
                                        min(1, |(x, y)|): a short (x, y) has an ill-conditioned angle
  a keypoint's d2 against 0 and r * r   min(d2, |d2 - r2|) / r2
"""
import numpy as np

BINS, WIDTH = 11, 33


def has_normal(normals):
    """normals f64 [3,N] -> bool [N]"""
    return np.isfinite(normals).all(0) & (normals != 0.0).any(0)


def _edge_margin(t):
    """distance of t in [0, 11] to the nearest of the inner edges 1 .. 10"""
    return np.abs(t[..., None] - np.arange(1.0, 11.0)).min(-1)


def spfh(pc, normals, radius, count=None):
    """pc f32 [3,N], normals f64 [3,N] -> (spfh i64 [N,33], members i64 [N], margin)"""
    N = pc.shape[1]
    n = N if count is None else int(np.clip(count, 0, N))
    out, members = np.zeros((N, WIDTH), np.int64), np.zeros(N, np.int64)
    P = pc.T.astype(np.float64)[:n]
    nr = normals.T.astype(np.float64)[:n]
    ok = has_normal(normals)[:n]
    idx = np.nonzero(ok)[0]
    if idx.size < 2:
        return out, members, np.inf
    P, nr = P[idx], nr[idx]
    r2 = np.float64(radius) * np.float64(radius)
    D = P[None, :, :] - P[:, None, :]                                  # D[i, j] = p_j - p_i
    d2 = np.sum(D * D, -1)
    off = ~np.eye(idx.size, dtype=bool)
    margin = (np.abs(d2 - r2) / r2)[off].min()
    member = (d2 < r2) & off
    members[idx] = member.sum(1)
    i, j = np.nonzero(member)
    if i.size == 0:
        return out, members, margin
    d, ni, nj = D[i, j], nr[i], nr[j]
    f4 = np.sqrt(d2[i, j])
    margin = min(margin, (f4 / radius).min())
    keep = f4 > 0.0
    i, d, ni, nj, f4 = i[keep], d[keep], ni[keep], nj[keep], f4[keep]
    a1, a2 = np.sum(ni * d, -1) / f4, np.sum(nj * d, -1) / f4
    big = np.maximum(np.abs(a1), np.abs(a2))
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = min(margin, np.where(big > 0.0, np.abs(np.abs(a1) - np.abs(a2)) / big, 0.0).min(initial=np.inf))
    swap = np.abs(a1) < np.abs(a2)
    n1, n2 = np.where(swap[:, None], nj, ni), np.where(swap[:, None], ni, nj)
    d = np.where(swap[:, None], -d, d)
    f3 = np.where(swap, -a2, a1)
    v = np.cross(d, n1)
    vn = np.sqrt(np.sum(v * v, -1))
    margin = min(margin, (vn / f4).min(initial=np.inf))
    keep = vn > 0.0
    i, n1, n2, f3, v, vn = i[keep], n1[keep], n2[keep], f3[keep], v[keep], vn[keep]
    v = v / vn[:, None]
    w = np.cross(n1, v)
    f2 = np.sum(v * n2, -1)
    y, x = np.sum(w * n2, -1) + 0.0, np.sum(n1 * n2, -1) + 0.0          # (-0.0 -> +0.0)
    t1 = BINS * (np.arctan2(y, x) + np.pi) / (2.0 * np.pi)
    t2, t3 = BINS * (f2 + 1.0) / 2.0, BINS * (f3 + 1.0) / 2.0
    margin = min(margin, (np.abs(t1 - np.round(t1)) * np.minimum(1.0, np.hypot(x, y))).min(initial=np.inf),
                 _edge_margin(t2).min(initial=np.inf), _edge_margin(t3).min(initial=np.inf))
    h1, h2, h3 = (np.clip(np.floor(t), 0, BINS - 1).astype(np.int64) for t in (t1, t2, t3))
    for h, base in ((h1, 0), (h2, BINS), (h3, 2 * BINS)):
        np.add.at(out, (idx[i], base + h), 1)
    return out, members, margin


def fpfh(pc, spfh_counts, members, keypoints, radius, count=None, kp_count=None):
    """pc f32 [3,N], spfh [N,33], members [N], keypoints f32 [3,M] -> (fpfh f64 [M,33], kp_members i64 [M], margin)"""
    N, M = pc.shape[1], keypoints.shape[1]
    n = N if count is None else int(np.clip(count, 0, N))
    m = M if kp_count is None else int(np.clip(kp_count, 0, M))
    out, kp_members = np.zeros((M, WIDTH)), np.zeros(M, np.int64)
    P = pc.T.astype(np.float64)[:n]
    r2 = np.float64(radius) * np.float64(radius)
    margin = np.inf
    for q in range(m):
        d = P - keypoints[:, q].astype(np.float64)
        d2 = np.sum(d * d, -1)
        if n:
            margin = min(margin, (np.minimum(d2, np.abs(d2 - r2)) / r2).min())
        mask = (members[:n] > 0) & (d2 > 0.0) & (d2 < r2)
        kp_members[q] = mask.sum()
        if not mask.any():
            continue
        terms = spfh_counts[:n][mask].astype(np.float64) * (100.0 / members[:n][mask])[:, None] / d2[mask][:, None]
        acc = np.sum(terms, 0)
        for h in range(3):
            s = np.sum(acc[h * BINS:(h + 1) * BINS])
            out[q, h * BINS:(h + 1) * BINS] = acc[h * BINS:(h + 1) * BINS] * (100.0 / s) if s > 0.0 else 0.0
    return out, kp_members, margin
