"""An independent numpy restatement of the SHOT-352 contract (include/usip_hip.h f-20) for tests/test_shot_cpu.py:
all pairs, np.linalg.eigh instead of the fixed-sweep Jacobi, np.arctan2 / np.arccos instead of the header's own inverse tangent,
float weights without a quantum, plain np.sum.  It shares no code with csrc/shot_math.h.

Every function also reports the smallest RELATIVE margin of each kind of decision it took, so that a test can assert, as a
condition on its input, that no decision sits on a threshold before it compares anything else:
  d2        |d2 - r2| / r2 over all (keypoint, live row) pairs
  dots      |d . x| / |d| and |d . z| / |d| over the frame's members (d != 0): the votes on the two signs
  votes     |#(d . a >= 0) - #(d . a < 0)| / members: no tie and no near tie
  eig       (l_k+1 - l_k) / l_max over the three eigenvalues
  cos       the distance of t + 0.5 from an integer
  shell     |dist - r / 2| / r
  half      |z'| / dist
  diag      ||x'| - |y'|| / dist
  axes      min(|x'|, |y'|) / dist
The member count against 5 is an integer decision: it rides on d2's margin."""
import numpy as np

WIDTH = 352
U = 2.0 ** -53


def has_normal(n):
    """n [3,N] -> bool [N]"""
    return np.isfinite(n).all(0) & (n != 0).any(0)


def _live(pc, count):
    return pc.shape[1] if count is None else max(0, min(int(count), pc.shape[1]))


def frames(pc, kp, radius, count=None, kp_count=None):
    """pc f32 [3,N], kp f32 [3,M] -> dict(lrf [M,9] (zeros without a frame), members [M], framed bool [M], gap [M,2] the
    relative gaps that isolate x and z, vote i32 [M] the smaller |#(>= 0) - #(< 0)| of the two sign votes, bar [M] the derived
    bound on |axis - exact axis|, margins {kind: value})"""
    n, m = _live(pc, count), _live(kp, kp_count)
    M = kp.shape[1]
    p = pc[:, :n].astype(np.float64).T
    lrf, members, framed = np.zeros((M, 9)), np.zeros(M, np.int32), np.zeros(M, bool)
    gap, bar, vote = np.full((M, 2), np.inf), np.zeros(M), np.full(M, 1 << 30, np.int32)
    mg = dict(d2=np.inf, dots=np.inf, votes=np.inf, eig=np.inf)
    r2 = radius * radius
    for q in range(m):
        d = p - kp[:, q].astype(np.float64)
        d2 = (d * d).sum(1)
        if n:
            mg["d2"] = min(mg["d2"], np.abs(d2 - r2).min() / r2)
        inside = d2 < r2
        members[q] = inside.sum()
        if members[q] < 5:
            continue
        d, dist = d[inside], np.sqrt(d2[inside])
        w = radius - dist
        W = w.sum()
        if not W > 0:
            continue
        C = (d * w[:, None]).T @ d / W
        lam, vec = np.linalg.eigh(C)
        mg["eig"] = min(mg["eig"], np.diff(lam).min() / lam[2])
        gap[q] = (lam[2] - lam[1]) / lam[2], (lam[1] - lam[0]) / lam[2]
        x, z = vec[:, 2], vec[:, 0]
        off = dist > 0
        for a in (x, z):
            dots = d @ a
            mg["dots"] = min(mg["dots"], (np.abs(dots[off]) / dist[off]).min())
            pos, neg = (dots >= 0).sum(), (dots < 0).sum()
            mg["votes"] = min(mg["votes"], abs(int(pos) - int(neg)) / members[q])
            vote[q] = min(vote[q], abs(int(pos) - int(neg)))
            if pos < neg:
                a *= -1.0
        lrf[q] = np.concatenate([x, np.cross(z, x), z])
        framed[q] = True
        # the bar: one side's seven sums against exact arithmetic.  A term w da db: da, db one rounding each, d2 five, its root
        # and the difference from r leave w with an ABSOLUTE error of at most 4.5 u r, the two products two more: at most
        # 9.5 u r |d|^2; k terms in any order add (k - 1) u: |dS| <= (k + 9) u R, R = sum r |d|^2.  W: at most (4.5 k r / W + k)
        # u relative.  Either eigen-solver: at most 64 u |C| (24 rotations, or LAPACK's).  Two sides; an eigenvector moves by at
        # most 2 |dC| / gap (Davis-Kahan).
        k = float(members[q])
        R = (radius * dist * dist).sum()
        normC = np.sqrt((C * C).sum())
        dC = 2.0 * U * ((k + 9.0) * R / W + (4.5 * k * radius / W + k) * normC + 64.0 * normC)
        bar[q] = 2.0 * dC / (min(gap[q]) * lam[2])
    return dict(lrf=lrf, members=members, framed=framed, gap=gap, vote=vote, bar=bar, margins=mg)


def histograms(pc, normals, kp, lrf, radius, eps_a, count=None, kp_count=None):
    """pc f32 [3,N], normals f64 [3,N], kp f32 [3,M], lrf f64 [M,9] (whoever's) -> dict(hist f64 [M,352] in units of one member's
    one dimension (a member adds 4 in all), hard i32 [M,352] the members per own column, kp_members [M], bar [M,352] the derived
    bound on |twin's hist / 2^32 - hist|, full bool [M]: no member of the keypoint lacks a neighbour; margins)"""
    n, m = _live(pc, count), _live(kp, kp_count)
    M = kp.shape[1]
    p = pc[:, :n].astype(np.float64).T
    nrm = normals[:, :n].T
    ok = has_normal(normals[:, :n])
    hist, hard, bar = np.zeros((M, WIDTH)), np.zeros((M, WIDTH), np.int32), np.zeros((M, WIDTH))
    kpm, full = np.zeros(M, np.int32), np.ones(M, bool)
    mg = dict(d2=np.inf, cos=np.inf, shell=np.inf, half=np.inf, diag=np.inf, axes=np.inf)
    r2, half = radius * radius, radius / 2.0
    for q in range(m):
        d = p - kp[:, q].astype(np.float64)
        d2 = (d * d).sum(1)
        if n:
            mg["d2"] = min(mg["d2"], np.abs(d2 - r2).min() / r2)
        sel = ok & (d2 < r2) & (d2 > 0)
        kpm[q] = sel.sum()
        F = lrf[q].reshape(3, 3)
        if not (np.isfinite(F).all() and (F[0] != 0).any()):
            continue
        for dj, nj, d2j in zip(d[sel], nrm[sel], d2[sel]):
            dist = np.sqrt(d2j)
            xp, yp, zp = F @ dj
            c = float(np.clip(nj @ F[2], -1.0, 1.0))
            t = (1.0 + c) * 5.0
            cb = int(np.floor(t + 0.5))
            phi = np.arctan2(yp, xp)
            az = min(int(np.floor((phi + np.pi) / (np.pi / 4.0))), 7)
            sh, el = int(dist > half), int(zp > 0)
            rho = np.hypot(xp, yp)
            mg["cos"] = min(mg["cos"], abs(t + 0.5 - np.round(t + 0.5)))
            mg["shell"] = min(mg["shell"], abs(dist - half) / radius)
            mg["half"] = min(mg["half"], abs(zp) / dist)
            mg["diag"] = min(mg["diag"], abs(abs(xp) - abs(yp)) / dist)
            mg["axes"] = min(mg["axes"], min(abs(xp), abs(yp)) / dist)
            col = lambda a, e, s, b: ((a * 2 + e) * 2 + s) * 11 + b             # noqa: E731
            own = col(az, el, sh, cb)
            adds = []
            dcos = t - cb
            if dcos != 0 and 0 <= cb + np.sign(dcos) <= 10:
                adds.append((col(az, el, sh, cb + int(np.sign(dcos))), abs(dcos)))
            drad = (dist - half) / half - 0.5 if sh else dist / half - 0.5
            if (drad < 0) if sh else (drad > 0):
                adds.append((col(az, el, 1 - sh, cb), abs(drad)))
            elif drad != 0:
                full[q] = False
            theta = np.arccos(np.clip(zp / dist, -1.0, 1.0))
            dele = (theta - (np.pi / 4.0 if el else 3.0 * np.pi / 4.0)) / (np.pi / 2.0)
            if (dele > 0) if el else (dele < 0):
                adds.append((col(az, 1 - el, sh, cb), abs(dele)))
            elif dele != 0:
                full[q] = False
            dazi = (phi - (-np.pi + (az + 0.5) * np.pi / 4.0)) / (np.pi / 4.0)
            if dazi != 0:
                adds.append((col((az + int(np.sign(dazi))) % 8, el, sh, cb), abs(dazi)))
            hist[q, own] += 4.0 - (abs(dcos) + abs(drad) + abs(dele) + abs(dazi))
            hard[q, own] += 1
            # one member's share of a column's bar: five quanta; the two inverse tangents against numpy's, 2 eps_a each, over
            # the bin widths pi / 4 and pi / 2; float64 roundings: the three dots and c carry about 4 u |d| (4 u |n|) each, which
            # an angle sees divided by rho = |(x', y')| -- (8 u dist / rho) (4 / pi + 2 / pi) -- the cosine times 5 (20 u |n| +
            # 8 u), the radial offset 8 u, the four divisions and differences 16 u more
            e = 5.0 * 2.0 ** -32 + 2.0 * eps_a * (4.0 / np.pi) + 2.0 * eps_a * (2.0 / np.pi) + U * (
                8.0 * dist / rho * (6.0 / np.pi) + 20.0 * max(1.0, float(np.sqrt(nj @ nj))) + 32.0)
            for cidx in [own] + [a for a, _ in adds]:
                bar[q, cidx] += e
            for cidx, wgt in adds:
                hist[q, cidx] += wgt
    return dict(hist=hist, hard=hard, kp_members=kpm, bar=bar, full=full, margins=mg)


def descriptor(hist):
    """hist [M,352] -> hist over its Euclidean norm, zeros where that is zero"""
    s = np.sqrt((hist * hist).sum(1, keepdims=True))
    return np.where(s > 0, hist / np.where(s > 0, s, 1.0), 0.0)
