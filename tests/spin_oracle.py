"""An independent numpy restatement of the spin-image contract (include/usip_hip.h f-21) for tests/test_spin_cpu.py:
all pairs, the distance from the axis as the length of a cross product (not a difference of squares), np.arcsin instead of
the header's own inverse tangent, float bilinear weights without a quantum, plain sums.  It shares no code with
csrc/spin_math.h.

It also reports, per keypoint and over all of them, the smallest margin of each kind of decision it took, so that a test can
assert, as a condition on its input, that no decision sits on a threshold before it compares anything else:
  d2        |d2 - r2| / r2 over all (keypoint, live row) pairs
  edge      |u - W| / W and ||v| - W| / W over the rows of the sphere (the rectangular structure's cylinder test)
  cell      the distance of u and of v from an integer, in bins, over the members
  support   ||n . a| - s| over the rows of the sphere with a normal (only with a support angle)"""
import numpy as np

W = 8
ROWS, COLS = W + 1, 2 * W + 1
WIDTH = ROWS * COLS
U = 2.0 ** -53
KINDS = ("d2", "edge", "cell", "support")


def has_normal(n):
    """n [3,N] -> bool [N]"""
    return np.isfinite(n).all(0) & (n != 0).any(0)


def _live(pc, count):
    return pc.shape[1] if count is None else max(0, min(int(count), pc.shape[1]))


def image(pc, kp, axes, radius, structure, eps_a, support=0.0, normals=None, count=None, kp_count=None):
    """pc f32 [3,N], kp f32 [3,M], axes f64 [M,3] (whoever's), normals f64 [3,N] with a support angle -> dict(hist f64 [M,153]
    in units of one member (a member adds 1 in all), cells i32 [M,8,16] the members per cell pair (ab, bb), kp_members [M], bar
    [M,153] the derived bound on |twin's hist / 2^40 - hist|, margin f64 [M] the smallest margin of the keypoint's
    decisions, margins {kind: the smallest over all keypoints})"""
    assert structure in ("rectangular", "radial")
    n, m = _live(pc, count), _live(kp, kp_count)
    M = kp.shape[1]
    p = pc[:, :n].astype(np.float64).T
    hist, bar = np.zeros((M, WIDTH)), np.zeros((M, WIDTH))
    cells, kpm = np.zeros((M, W, 2 * W), np.int32), np.zeros(M, np.int32)
    per = {k: np.full(M, np.inf) for k in KINDS}
    r2 = radius * radius
    for q in range(m):
        a = np.asarray(axes[q], np.float64)
        d = p - kp[:, q].astype(np.float64)
        d2 = (d * d).sum(1)
        if n:
            per["d2"][q] = np.abs(d2 - r2).min() / r2
        if not (np.isfinite(a).all() and a @ a > 0 and np.isfinite(a @ a)):
            continue
        a = a / np.linalg.norm(a)
        sel = (d2 < r2) & (d2 > 0)
        if support > 0:
            na = np.abs(normals[:, :n].T @ a)
            ok = has_normal(normals[:, :n])
            if (sel & ok).any():
                per["support"][q] = np.abs(na[sel & ok] - support).min()
            sel &= ok & ~(na < support)
        d, d2 = d[sel], d2[sel]
        dist, beta = np.sqrt(d2), d @ a
        alpha = np.linalg.norm(np.cross(d, a), axis=1)
        if structure == "rectangular":
            size = radius / np.sqrt(2.0) / W
            u, v = alpha / size, beta / size
            if len(u):
                per["edge"][q] = min(np.abs(u - W).min(), np.abs(np.abs(v) - W).min()) / W
            # the twin's alpha is sqrt(d2 - beta^2): d2 carries 4 u, beta 8 u dist per side, beta^2 17 u d2, the difference
            # 22 u d2 in all; |sqrt(x + e) - sqrt(x)| <= min(|e| / sqrt(x), sqrt(|e|)).  This side's cross product: 8 u dist.
            e = 22.0 * U * d2
            du = (np.minimum(e / np.maximum(alpha, 1e-300), np.sqrt(e)) + 8.0 * U * dist) / size + 8.0 * U * u
            dv = 16.0 * U * dist / size + 8.0 * U * np.abs(v)
            inside = (u < W) & (v < W) & (v > -W)
            u, v, du, dv = u[inside], v[inside], du[inside], dv[inside]
        else:
            size = radius / W
            u = dist / size
            c = np.clip(beta / dist, -1.0, 1.0)
            v = np.arcsin(c) / (np.pi / 2.0 / W)
            # c: 8 u per side from beta, the division and the root of d2: 20 u.  The arc sine moves by at most dc over the
            # smallest sqrt(1 - c^2) of the interval, and never by more than (pi / 2) sqrt(dc); the twin's root and its inverse
            # tangent's arguments add 4 u, the inverse tangent itself 2 eps_a against numpy's.
            dc = 20.0 * U
            top = np.abs(c) + dc
            slope = np.where(top < 1.0, dc / np.sqrt(np.maximum(1.0 - top * top, 1e-300)), np.inf)
            dtheta = np.minimum(slope, (np.pi / 2.0) * np.sqrt(dc)) + 2.0 * eps_a + 4.0 * U
            du = 8.0 * U * u
            dv = dtheta * (W / (np.pi / 2.0)) + 4.0 * U * np.abs(v)
        kpm[q] = len(u)
        if not len(u):
            continue
        per["cell"][q] = min(np.abs(u - np.round(u)).min(), np.abs(v - np.round(v)).min())
        ab, bb = np.floor(u).astype(int), np.floor(v).astype(int) + W
        fa, fb = u - np.floor(u), v - np.floor(v)
        over = ab >= W                                                  # the radial structure's border rule
        ab[over], fa[over] = W - 1, 1.0
        over = bb >= 2 * W
        bb[over], fb[over] = 2 * W - 1, 1.0
        np.add.at(cells[q], (ab, bb), 1)
        # a member's share of a cell's bar: the two truncations of 2^-20, and the roundings of u and v (a bilinear weight
        # moves by at most the sum of the two offsets' moves)
        e = 2.0 * 2.0 ** -20 + du + dv
        for da, db, wgt in ((0, 0, (1 - fa) * (1 - fb)), (1, 0, fa * (1 - fb)), (0, 1, (1 - fa) * fb), (1, 1, fa * fb)):
            np.add.at(hist[q], (ab + da) * COLS + bb + db, wgt)
            np.add.at(bar[q], (ab + da) * COLS + bb + db, e)
    margin = np.min([per[k] for k in KINDS], axis=0)
    return dict(hist=hist, cells=cells, kp_members=kpm, bar=bar, margin=margin, margins={k: per[k].min() for k in KINDS})


def descriptor(hist, kp_members):
    """hist [M,153] in members -> the image over its member count, zeros where that is zero"""
    k = np.maximum(kp_members, 1)[:, None].astype(np.float64)
    return np.where(kp_members[:, None] > 0, hist / k, 0.0)
