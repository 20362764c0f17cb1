"""A plain numpy restatement of the f-12 contract (include/usip_hip.h: Fast Global Registration of one fragment pair), and
the fixtures the host and device tests share.  Independent of the library: numpy.mean, numpy.einsum, numpy.linalg,
numpy.sin / numpy.cos, explicit triples (there is no Philox here).  Sums are numpy's, not the contract's lane-strided tree,
so values agree with the library to rounding only; `reverse` feeds the rows to the sums in reversed order, which measures
that rounding.  Every decision on an inequality reports its margin, so a test can first assert that the decision does not
hang on rounding.

Each fixture ASSERTS the property it exists for (fixture() does it on the oracle's own result), so that an edit of its
parameters cannot quietly turn it into an easy input."""
import functools

import numpy as np

TRIALS_PER_ROW, TUPLE_CAP, MIN_ROWS, TUPLE_SCALE = 100, 1000, 10, 0.95
ITERATIONS, DIV_FACTOR, MAX_CORR_DIST, THRESHOLD, CHUNK = 64, 1.4, 0.025, 0.2, 256


def nearest(a, b, na, nb):
    """a [C,Ma], b [C,Mb] float32 -> i32 [Ma]: the first nearest column of b[:, :nb] for every column of a[:, :na], 0 beyond"""
    out = np.zeros(a.shape[1], np.int32)
    if na > 0 and nb > 0:
        d = ((a[:, :na, None].astype(np.float64) - b[:, None, :nb].astype(np.float64)) ** 2).sum(0)
        out[:na] = np.argmin(d, axis=1)
    return out


def mutual_rows(n1, n2, nn12, nn21):
    n1, n2 = int(np.clip(n1, 0, len(nn12))), int(np.clip(n2, 0, len(nn21)))
    return np.array([(i, nn12[i]) for i in range(n1) if 0 <= nn12[i] < n2 and nn21[nn12[i]] == i], np.int64).reshape(-1, 2)


def random_triples(rng, nc, T=None):
    """i32 [T,3]: three distinct rows of [0, nc) per trial (zeros when there are fewer than three rows)"""
    T = TRIALS_PER_ROW * nc if T is None else T
    if nc < 3:
        return np.zeros((max(T, 1), 3), np.int32)
    a = rng.integers(0, nc, T)
    b = (a + rng.integers(1, nc, T)) % nc
    c = rng.integers(0, nc - 2, T)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    c = c + (c >= lo)
    c = c + (c >= hi)
    return np.stack((a, b, c), 1).astype(np.int32)


def rotation(x):
    sa, ca, sb, cb, sg, cg = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def register(kp1, kp2, n1, n2, nn12, nn21, triples, threshold=THRESHOLD, reverse=False):
    """One pair: kp f32 [3,M], triples i32 [T,3] -> dict.  edge_margin: the smallest |ratio - bound| over every edge test
    that was evaluated (lj / li against 0.95 and 1 / 0.95); residual_margin: the smallest | residual - threshold |."""
    M = kp1.shape[1]
    n1, n2 = int(np.clip(n1, 0, M)), int(np.clip(n2, 0, M))
    mutual = mutual_rows(n1, n2, nn12, nn21)
    nc = len(mutual)
    a, b = kp1.astype(np.float64), kp2.astype(np.float64)
    m1 = a[:, :n1].mean(1) if n1 else np.zeros(3)
    m2 = b[:, :n2].mean(1) if n2 else np.zeros(3)
    norms = np.concatenate((np.sqrt(((a[:, :n1] - m1[:, None]) ** 2).sum(0)), np.sqrt(((b[:, :n2] - m2[:, None]) ** 2).sum(0))))
    scale = float(norms.max()) if len(norms) else 0.0
    out = dict(mutual=mutual, nc=nc, mean1=m1, mean2=m2, scale=scale, rows=np.zeros(0, np.int64), row_count=0,
               trials_walked=0, Rt=np.eye(3, 4), valid=0, inlier_mask=np.zeros(M, np.uint8), inliers=0, edge_margin=np.inf,
               residual_margin=np.inf, T=0, accepted=0)
    if not (np.isfinite(scale) and scale > 0):
        return out
    u1 = (a[:, mutual[:, 0]] - m1[:, None]).T / scale                  # [nc,3]
    u2 = (b[:, mutual[:, 1]] - m2[:, None]).T / scale
    T = min(TRIALS_PER_ROW * nc, len(triples))
    out["T"] = T
    rows, walked, margin = [], T, np.inf
    if T:
        tr = np.clip(triples[:T].astype(np.int64), 0, nc - 1)
        acc = np.ones(T, bool)
        for x, y in ((0, 1), (0, 2), (1, 2)):
            li = np.sqrt(((u1[tr[:, x]] - u1[tr[:, y]]) ** 2).sum(1))
            lj = np.sqrt(((u2[tr[:, x]] - u2[tr[:, y]]) ** 2).sum(1))
            acc &= (li * TUPLE_SCALE < lj) & (lj < li / TUPLE_SCALE)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = lj / li
            ratio = ratio[np.isfinite(ratio)]
            if len(ratio):
                margin = min(margin, np.abs(ratio - TUPLE_SCALE).min(), np.abs(ratio - 1 / TUPLE_SCALE).min())
        hits = np.nonzero(acc)[0]
        out["accepted"] = len(hits)
        if len(hits) >= TUPLE_CAP:
            hits = hits[:TUPLE_CAP]
            walked = int(hits[-1]) + 1
        rows = tr[hits].reshape(-1)
    out.update(rows=np.asarray(rows, np.int64), row_count=len(rows), trials_walked=walked, edge_margin=margin)
    if len(rows) < MIN_ROWS:
        return out
    order = rows[::-1] if reverse else rows
    p, q0 = u1[order], u2[order]
    R, t, par = np.eye(3), np.zeros(3), 1.0
    for k in range(ITERATIONS):
        if k % 4 == 0 and par > MAX_CORR_DIST:
            par = par / DIV_FACTOR
        q = q0 @ R.T + t
        r = p - q
        e = (r ** 2).sum(1)
        s = (par / (e + par)) ** 2
        J = np.zeros((len(q), 3, 6))
        J[:, 0, 1], J[:, 0, 2], J[:, 0, 3] = -q[:, 2], q[:, 1], -1
        J[:, 1, 0], J[:, 1, 2], J[:, 1, 4] = q[:, 2], -q[:, 0], -1
        J[:, 2, 0], J[:, 2, 1], J[:, 2, 5] = -q[:, 1], q[:, 0], -1
        A = np.einsum("n,nki,nkj->ij", s, J, J)
        g = np.einsum("n,nki,nk->i", s, J, r)
        try:
            np.linalg.cholesky(A)
            x = -np.linalg.solve(A, g)
        except np.linalg.LinAlgError:
            return out
        if not np.isfinite(x).all() or (np.abs(x[:3]) > np.pi).any():
            return out
        Rd = rotation(x)
        R, t = Rd @ R, Rd @ t + x[3:]
    Rt = np.concatenate((R, (-R @ m2 + t * scale + m1)[:, None]), 1)
    res = np.sqrt(((a[:, mutual[:, 0]] - (Rt[:, :3] @ b[:, mutual[:, 1]] + Rt[:, 3:])) ** 2).sum(0))
    mask = np.zeros(M, np.uint8)
    mask[:nc] = res < threshold
    out.update(Rt=Rt, valid=1, inlier_mask=mask, inliers=int(mask.sum()),
               residual_margin=float(np.abs(res - threshold).min()) if nc else np.inf)
    return out


# ------------------------------------------------------------------------------------------------ fixtures
def planted(seed, M, shared, n1=None, n2=None, noise=0.01, dim=32, identical=False):
    """Two fragments of M uniform points in a 5 m cube; the first `shared` of either are the same points under a rotation
    and a shift (1 cm noise on fragment 2) and carry the same descriptor; the others are unrelated.  -> dict(kp1, kp2 f32
    [3,M], d1, d2 f32 [dim,M], n1, n2, gt f64 [3,4] with x1 = R x2 + t)."""
    rng = np.random.default_rng(seed)
    w1 = rng.uniform(0, 5, (M, 3))
    w2 = np.concatenate((w1[:shared], rng.uniform(0, 5, (M - shared, 3))))
    code = rng.normal(size=(2 * M, dim))
    code /= np.linalg.norm(code, axis=1, keepdims=True)
    d1, d2 = code[:M].copy(), np.concatenate((code[:shared], code[M + shared:]))
    R = rotation(rng.uniform(-0.6, 0.6, 3))
    t = rng.uniform(-1, 1, 3)
    if identical:
        w2, d2, R, t, noise = w1.copy(), d1.copy(), np.eye(3), np.zeros(3), 0.0
    x2 = (w2 - t) @ R + rng.normal(scale=noise, size=w2.shape) if noise else (w2 - t) @ R      # R'(x1 - t)
    mix1, mix2 = rng.permutation(M), rng.permutation(M)                # the shared points sit anywhere in either list
    kp1, kp2 = np.ascontiguousarray(w1[mix1].T, np.float32), np.ascontiguousarray(x2[mix2].T, np.float32)
    d1, d2 = np.ascontiguousarray(d1[mix1].T, np.float32), np.ascontiguousarray(d2[mix2].T, np.float32)
    return dict(kp1=kp1, kp2=kp2, d1=d1, d2=d2, n1=M if n1 is None else n1, n2=M if n2 is None else n2,
                gt=np.concatenate((R, t[:, None]), 1))


def finish(f, seed, nn=None):
    """adds nn12, nn21 (the nearest descriptors, or `nn` as given), the triples of seed `seed` and the oracle's results"""
    M = f["kp1"].shape[1]
    c1, c2 = int(np.clip(f["n1"], 0, M)), int(np.clip(f["n2"], 0, M))
    f["nn12"], f["nn21"] = nn if nn is not None else (nearest(f["d1"], f["d2"], c1, c2), nearest(f["d2"], f["d1"], c2, c1))
    nc = len(mutual_rows(f["n1"], f["n2"], f["nn12"], f["nn21"]))
    f["triples"] = random_triples(np.random.default_rng(seed), nc)
    f["oracle"] = register(f["kp1"], f["kp2"], f["n1"], f["n2"], f["nn12"], f["nn21"], f["triples"])
    f["oracle_reversed"] = register(f["kp1"], f["kp2"], f["n1"], f["n2"], f["nn12"], f["nn21"], f["triples"], reverse=True)
    return f


def pose_error(o, gt):
    """the largest entry of | R - R_gt | and of | t - t_gt | / scale"""
    return max(np.abs(o["Rt"][:, :3] - gt[:, :3]).max(), np.abs(o["Rt"][:, 3] - gt[:, 3]).max() / o["scale"])


def _few_rows_seed():
    """M = 32 with 3 planted: the first seed whose tuple test accepts something, but fewer than MIN_ROWS rows"""
    for seed in range(200):
        f = finish(planted(300 + seed, 32, 3), 301 + seed)
        if 0 < f["oracle"]["row_count"] < MIN_ROWS:
            return f
    raise AssertionError("no seed below 200 gives 0 < row_count < %d" % MIN_ROWS)


NAMES = ("cap", "sparse", "few_rows", "unrelated", "nc0", "nc1", "nc2", "empty1", "coincident", "identical", "limit",
         "bad_index", "counts_beyond")


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name == "cap":                  # the cap of 1000 fills inside a chunk, before the trials end
        f = finish(planted(12, 64, 32), 13)
        o = f["oracle"]
        assert o["row_count"] == 3 * TUPLE_CAP and o["trials_walked"] < o["T"] and o["trials_walked"] % CHUNK != 0, o
        assert o["valid"] and pose_error(o, f["gt"]) < 2e-3, pose_error(o, f["gt"])
    elif name == "sparse":             # the cap does not fill; T is no multiple of the chunk
        f = finish(planted(36, 48, 6), 37)
        o = f["oracle"]
        assert 13 <= o["nc"] <= 20 and MIN_ROWS <= o["row_count"] < 3 * TUPLE_CAP, (o["nc"], o["row_count"])
        assert o["trials_walked"] == o["T"] == 100 * o["nc"] and o["T"] % CHUNK != 0
        assert o["valid"] and pose_error(o, f["gt"]) < 0.02, pose_error(o, f["gt"])
    elif name == "few_rows":           # something accepted, fewer than 10 rows: invalid, [I | 0]
        f = _few_rows_seed()
        o = f["oracle"]
        assert 0 < o["row_count"] < MIN_ROWS and not o["valid"] and (o["Rt"] == np.eye(3, 4)).all()
    elif name == "unrelated":          # no planted partner: no accepted trial
        f = finish(planted(41, 32, 0), 42)
        o = f["oracle"]
        assert o["nc"] >= 3 and o["accepted"] == 0 and o["trials_walked"] == o["T"] and not o["valid"], (o["nc"], o["accepted"])
    elif name in ("nc0", "nc1", "nc2"):
        want = int(name[2])
        f = planted(51, 16, 8)
        nn12 = ((np.arange(16) + 1) % 16).astype(np.int32)            # i -> i + 1 -> i + 2: never mutual
        nn21 = nn12.copy()
        for i in range(want):
            nn12[i], nn21[i] = i, i
        f = finish(f, 52, (nn12, nn21))
        o = f["oracle"]
        assert o["nc"] == want and o["row_count"] == 0 and o["trials_walked"] == 100 * want and not o["valid"], o
    elif name == "empty1":             # n1 = 0
        f = finish(planted(61, 16, 8, n1=0), 62)
        assert f["oracle"]["nc"] == 0 and f["oracle"]["scale"] > 0 and not f["oracle"]["valid"]
    elif name == "coincident":         # every point of both fragments at its fragment's mean: scale == 0
        f = planted(71, 16, 8)
        f["kp1"][:] = np.float32(1.25)
        f["kp2"][:] = np.float32(-0.5)
        f = finish(f, 72)
        o = f["oracle"]
        assert o["nc"] >= 3 and o["scale"] == 0 and o["trials_walked"] == 0 and not o["valid"]
    elif name == "identical":          # identical fragments: the identity
        f = finish(planted(81, 40, 40, identical=True), 82)
        o = f["oracle"]
        assert o["nc"] == 40 and o["valid"] and o["inliers"] == 40
    elif name == "limit":              # M = 1024, a 30 % share
        f = finish(planted(91, 1024, 307), 92)
        o = f["oracle"]
        assert 307 <= o["nc"] <= 1024 and o["valid"] and o["row_count"] == 3 * TUPLE_CAP, (o["nc"], o["row_count"])
    elif name == "bad_index":          # nn12 entries outside [0, n2) make no row
        f = planted(12, 64, 32)
        c1 = nearest(f["d1"], f["d2"], 64, 64)
        c2 = nearest(f["d2"], f["d1"], 64, 64)
        full = len(mutual_rows(64, 64, c1, c2))
        hit = [i for i in range(64) if c2[c1[i]] == i][:3]
        c1[hit[0]], c1[hit[1]], c1[hit[2]] = -1, 64, 2 ** 30
        f = finish(f, 102, (c1, c2))
        assert f["oracle"]["nc"] == full - 3 and f["oracle"]["valid"]
    elif name == "counts_beyond":      # a count above M behaves as M, one below 0 as 0
        f = finish(planted(12, 64, 32, n1=1000, n2=64), 13)
        g = fixture("cap")["oracle"]
        assert f["oracle"]["nc"] == g["nc"] and (f["oracle"]["Rt"] == g["Rt"]).all()
    else:
        raise KeyError(name)
    return f


def noise():
    """The oracle's own summation noise: the largest | Rt(rows forward) - Rt(rows reversed) | over the fixtures."""
    return max(float(np.abs(fixture(n)["oracle"]["Rt"] - fixture(n)["oracle_reversed"]["Rt"]).max()) for n in NAMES)
