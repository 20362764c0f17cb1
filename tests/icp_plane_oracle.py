"""A plain numpy restatement of the f-28 contract (include/usip_hip.h: trimmed ICP under the point-to-plane metric), and the
fixtures the host and device tests share.  The loop around the fit is tests/icp_oracle.py's own -- its move, its brute-force
nearest neighbour, its lexsort trim, its stopping rule and final pass -- so distances carry the library's bits.  The fit is
numpy's: the 27 sums by a matrix product, the step by numpy.linalg.solve (numpy.linalg.cholesky says whether the pivots are
positive), the rotation Rz Ry Rx from numpy's sine and cosine.  Poses therefore agree with the library to rounding only;
`reverse` feeds the kept rows to the sums in reversed order and `lstsq` replaces the solve, which together measure that
rounding (noise()).

Normals: normals() is the brute-force restatement of the scan preparation's (the 9 nearest OTHER rows, the covariance about
the row, numpy.linalg.eigh), compared with the library's up to sign in tests/test_icp_plane_cpu.py.  The room fixtures feed
the loop the LIBRARY's float32 normals (the host twin's, usip_amd.prepare.normals_cpu), as the issue of f-28 asks: the
fit's input is then the same on both sides.  The other fixtures plant their normals.

Each fixture ASSERTS the property it exists for on the oracle's own result."""
import functools
import math

import numpy as np

import icp_oracle as io

K = 9
Q = io.Q


# ------------------------------------------------------------------------------------------------ normals
def normals(xyz, k=K):
    """float32 [n,3], n > k -> (f64 [n,3] unit normals of arbitrary sign, gap [n]: (l1 - l0) / l2 of the covariance's
    ascending eigenvalues -- where it is tiny the normal is not determined)"""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    d = io.sqdist(p, p)
    d[np.arange(len(p)), np.arange(len(p))] = np.inf                   # the row itself is left out by index
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    e = p[nn] - p[:, None, :]
    C = np.einsum("nki,nkj->nij", e, e) / k
    w, v = np.linalg.eigh(C)
    return v[:, :, 0], (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0)


def library_normals(xyz):
    """float32 [n,3] -> float32 [n,3]: the host twin's, towards the origin; zeros below k + 1 rows (RefineBank's rule)"""
    from usip_amd import prepare
    a = np.asarray(xyz, np.float32)
    if len(a) < K + 1:
        return np.zeros((len(a), 3), np.float32)
    xyzi = np.ascontiguousarray(np.concatenate((a, np.zeros((len(a), 1), np.float32)), 1))
    return np.ascontiguousarray(prepare.normals_cpu(xyzi, None, K, (0.0, 0.0, 0.0))[2][:, :3])


# ------------------------------------------------------------------------------------------------ the contract
def rotation_zyx(x):
    sa, ca, sb, cb, sg, cg = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], [-sb, cb * sa, cb * ca]])


def sums(A6, q, idx, kept, reverse=False):
    """-> f64 [27]: H_jk (j <= k, row-major), then g_j, over the kept rows"""
    rows = kept[::-1] if reverse else kept
    a, n, qk = A6[idx[rows], :3].astype(np.float64), A6[idx[rows], 3:6].astype(np.float64), q[rows]
    c = np.stack((qk[:, 1] * n[:, 2] - qk[:, 2] * n[:, 1], qk[:, 2] * n[:, 0] - qk[:, 0] * n[:, 2],
                  qk[:, 0] * n[:, 1] - qk[:, 1] * n[:, 0]), 1)
    J = np.concatenate((c, n), 1)
    r = ((qk[:, 0] - a[:, 0]) * n[:, 0] + (qk[:, 1] - a[:, 1]) * n[:, 1]) + (qk[:, 2] - a[:, 2]) * n[:, 2]
    H = J.T @ J
    return np.concatenate((H[np.triu_indices(6)], J.T @ r))


def solve(S, lstsq=False):
    """-> (x or None when the solve fails, the relative margin of the decision)"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = S[:21]
    H = H + np.triu(H, 1).T
    w = np.linalg.eigvalsh(H)
    margin = float(w[0] / w[-1]) if w[-1] > 0 else 0.0
    try:
        np.linalg.cholesky(H)                                          # the pivots: finite and positive, or no step
        x = np.linalg.lstsq(H, -S[21:], rcond=None)[0] if lstsq else np.linalg.solve(H, -S[21:])
    except np.linalg.LinAlgError:
        return None, margin
    if not np.isfinite(x).all() or np.abs(x[:3]).max() > math.pi:
        return None, margin
    return x, min(margin, float((math.pi - np.abs(x[:3]).max()) / math.pi))


def refine(A6, B, Rt0, inlier_ratio=io.INLIER_RATIO, max_iterations=io.ITERATIONS, tolerance=io.TOLERANCE,
           align_radius=io.RADIUS, reverse=False, lstsq=False):
    """icp_oracle.refine with the plane fit: A6 float32 [n1,6] (x y z nx ny nz), B float32 [n2,>=3] -> its dict plus sums
    (every fit's 27, the failed one included), failed, solve_margin"""
    A6, B = np.asarray(A6, np.float32), np.asarray(B, np.float32)[:, :3]
    A = np.ascontiguousarray(A6[:, :3])
    Rt0 = np.asarray(Rt0, np.float64).reshape(3, 4)
    n1, n2 = len(A), len(B)
    out = dict(Rt=Rt0.copy(), iterations=0, converged=0, hits=0, ratio=(0.0, 0.0), rmse=0.0, idx=np.zeros(n2, np.int32),
               d2=np.zeros(n2), kept=np.zeros(0, np.int64), nn_margin=np.inf, cut_margin=np.inf, stop_margin=np.inf,
               radius_margin=np.inf, solve_margin=np.inf, refined=0, kept_history=[], idx_history=[], cut_i=[], sums=[],
               failed=0)
    if n1 == 0 or n2 == 0:
        return out
    tol_t, tol_c = float(tolerance[0]), io.chordal(float(tolerance[1]))
    Rt, dts, dcs = Rt0.copy(), [], []
    out["refined"] = 1
    for k in range(1, max_iterations + 1):
        q = io.move(Rt, B)
        idx, d2, m_nn = io.nearest(A, q)
        kept, m_cut, icut = io.trim(d2, inlier_ratio)
        out["cut_i"].append(icut)
        out["nn_margin"], out["cut_margin"] = min(out["nn_margin"], m_nn), min(out["cut_margin"], m_cut)
        out["kept_history"].append(kept)
        out["idx_history"].append(idx)
        S = sums(A6, q, idx, kept, reverse)
        out["sums"].append(S)
        x, margin = solve(S, lstsq)
        if x is None:
            out["failed"] = 1
            break
        out["solve_margin"] = min(out["solve_margin"], margin)
        D = rotation_zyx(x)
        new = np.concatenate((D @ Rt[:, :3], (D @ Rt[:, 3] + x[3:])[:, None]), 1)
        dts.append(float(np.sqrt(((new[:, 3] - Rt[:, 3]) ** 2).sum())))
        dcs.append(float(np.sqrt(((new[:, :3] - Rt[:, :3]) ** 2).sum())))
        Rt = new
        out["iterations"] = k
        mt, mc = float(np.mean(dts[-3:])), float(np.mean(dcs[-3:]))
        for v, tol in ((mt, tol_t), (mc, tol_c)):
            if tol > 0:
                out["stop_margin"] = min(out["stop_margin"], abs(v - tol) / tol)
        if mt <= tol_t and mc <= tol_c:
            out["converged"] = 1
            break
    idx, d2, m_nn = io.nearest(A, io.move(Rt, B))
    kept, m_cut, icut = io.trim(d2, inlier_ratio)
    out["final_cut_i"] = icut
    dist = np.sqrt(d2)
    hits = int((dist < align_radius).sum())
    out.update(Rt=Rt, idx=idx, d2=d2, kept=kept, hits=hits, ratio=(hits / n1, hits / n2),
               rmse=float(np.sqrt(d2[kept].mean())), nn_margin=min(out["nn_margin"], m_nn),
               cut_margin=min(out["cut_margin"], m_cut),
               radius_margin=float((np.abs(dist - align_radius) / align_radius).min()), dt=dts, dc=dcs)
    return out


# ------------------------------------------------------------------------------------------------ fixtures
def with_normals(xyz, nrm):
    return np.ascontiguousarray(np.concatenate((np.asarray(xyz, np.float32), np.asarray(nrm, np.float32)), 1))


def lattice_plane(n2, grid=14):
    """Fragment 1: three coordinate planes, on each a grid x grid lattice of rows 8 units (of 1/64) apart with the plane's
    exact normal, its sign alternating from row to row.  The queries are n2 of those rows moved by s (1, -1, 1) units, s = 1 or
    2: each is nearest its own row (d2 = 3 s^2 against at least 44 to any other), its residual is +-s / 64, every J entry an
    integer / 64 and every term of every sum an integer / 4096 -- exact, so the 27 sums of the FIRST fit do not depend on
    the order of the additions.  The start is a quarter turn about z plus an integer shift, so the move is exact too."""
    rows, nrm = [], []
    for i in range(1, grid + 1):
        for j in range(1, grid + 1):
            sign = 1.0 if (i + j) % 2 else -1.0
            rows += [(8 * i, 8 * j, 0), (8 * i, 0, 8 * j), (0, 8 * i, 8 * j)]
            nrm += [(0, 0, sign), (0, -sign, 0), (sign, 0, 0)]
    A, N = np.array(rows, np.float64), np.array(nrm, np.float64)
    order = np.random.default_rng(7).permutation(len(A))
    A, N = A[order], N[order]
    pick = np.random.default_rng(8).permutation(len(A))[:n2]
    s = 1.0 + (np.arange(n2) % 2)
    q = A[pick] + s[:, None] * np.array([1.0, -1.0, 1.0])
    R, t = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([3.0, -2, 1])
    B = (q * Q - t) @ R
    Rt0 = np.concatenate((R, t[:, None]), 1)
    A32, B32 = (A * Q).astype(np.float32), B.astype(np.float32)
    assert np.array_equal(A32.astype(np.float64), A * Q) and np.array_equal(B32.astype(np.float64), B)
    assert np.array_equal(io.move(Rt0, B32), q * Q)
    return dict(A=with_normals(A32, N), B=with_normals(B32, np.tile([[0.0, 0.0, 1.0]], (n2, 1))), Rt0=Rt0, pick=pick, s=s)


def walls(planes, n1=300, n2=120, seed=41):
    """Fragment 1 on the planes x = 1 (normal e_x) and, with planes = 2, y = 1 (normal e_y); fragment 2 a subset moved a
    little.  One wall: c0 = q1 0 - q2 0 is an exact zero in every row, so H_00 = 0 and the FIRST pivot is exactly 0.  Two
    walls: n_z = 0 in every row, so column 5 of H is exactly zero and the LAST pivot is 0 - 0."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2, n1), rng.uniform(0, 2, n1)
    on_y = (np.arange(n1) % planes) == 1
    A = np.where(on_y[:, None], np.stack((u, np.ones(n1), v), 1), np.stack((np.ones(n1), u, v), 1))
    N = np.where(on_y[:, None], [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    B = A[rng.permutation(n1)[:n2]] + rng.normal(0, 0.01, (n2, 3))
    return dict(A=with_normals(A, N), B=with_normals(B, np.tile([[1.0, 0.0, 0.0]], (n2, 1))),
                Rt0=io.random_pose(rng, 0.01, 0.01)[:3])


ROOMS = tuple(io.ROOMS)
LATTICES = {"lattice_plane": (400, io.INLIER_RATIO), "lattice_255": (255, 1.0), "lattice_256": (256, 1.0),
            "lattice_257": (257, 1.0), "lattice_515": (515, 1.0)}
FAILING = ("one_wall", "two_walls", "one_row_b", "three_rows_b", "few_rows_a")
NOT_REFINED = ("empty_a", "empty_b", "masked")
NAMES = ROOMS + tuple(LATTICES) + FAILING + NOT_REFINED
TIGHT_NAMES = io.TIGHT_NAMES


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> dict(A f32 [n1,6], B f32 [n2,6], Rt0 f64 [3,4], mask, args (refine's keywords), oracle)"""
    mask, args = 1, {}
    if name in ROOMS:
        g = io.fixture(name)
        f = dict(A=with_normals(g["A"], library_normals(g["A"])), B=with_normals(g["B"], library_normals(g["B"])),
                 Rt0=g["Rt0"], true=g["true"])
    elif name in LATTICES:
        f = lattice_plane(LATTICES[name][0])
        args = dict(inlier_ratio=LATTICES[name][1], max_iterations=1)   # one fit: only the start pose is exact
    elif name in ("one_wall", "two_walls"):
        f = walls(1 if name == "one_wall" else 2)
    elif name in ("one_row_b", "three_rows_b"):                         # m = 1: one row cannot hold six unknowns
        f = walls(1)
        f["B"] = f["B"][:1 if name == "one_row_b" else 3]
    elif name == "few_rows_a":                                          # below the normals' limit: RefineBank's zeros
        rng = np.random.default_rng(43)
        a = rng.uniform(0, 1, (K, 3)).astype(np.float32)
        f = dict(A=with_normals(a, library_normals(a)), B=with_normals(rng.uniform(0, 1, (40, 3)), np.zeros((40, 3))),
                 Rt0=io.random_pose(rng, 0.05, 0.05)[:3])
    else:
        g = io.fixture(name)
        unit = np.tile([[0.0, 0.6, 0.8]], (max(len(g["A"]), len(g["B"])), 1))
        f = dict(A=with_normals(g["A"], unit[:len(g["A"])]), B=with_normals(g["B"], unit[:len(g["B"])]), Rt0=g["Rt0"])
        mask = g["mask"]
    f.update(mask=mask, args=args, name=name)
    o = refine(f["A"], f["B"], f["Rt0"], **args) if mask else refine(f["A"][:0], f["B"], f["Rt0"])
    f["oracle"] = o
    n2 = len(f["B"])
    if name in ROOMS:
        assert not o["failed"] and o["iterations"] >= 1, (name, o["iterations"])
    if name in LATTICES:
        assert not o["failed"] and o["iterations"] == 1 and len(o["sums"]) == 1
        k0 = o["kept_history"][0]
        assert len(k0) == io.trim_count(LATTICES[name][1], n2) and (name == "lattice_plane") == (len(k0) < n2)
        assert np.array_equal(o["idx_history"][0], f["pick"])           # every query is nearest its own row
        S = o["sums"][0] * 4096.0
        assert np.array_equal(S, np.rint(S)) and np.abs(S).max() < 2.0 ** 40        # integers / 4096: exact in any order
        assert np.array_equal(bits(o["sums"][0]), bits(sums(f["A"], io.move(f["Rt0"], f["B"][:, :3]), f["pick"], k0, True)))
        assert o["sums"][0][21:].all()                                  # every component of g is fed
    if name in FAILING:
        assert o["refined"] and o["failed"] and o["iterations"] == 0 and np.array_equal(o["Rt"], f["Rt0"]) and o["hits"] >= 0
        S = o["sums"][0]
        if name in ("one_wall", "one_row_b", "three_rows_b"):
            assert S[0] == 0.0 and S[15] > 0.0                         # H_00: the first pivot; H_33 = sum n_x n_x is there
        if name == "two_walls":
            assert S[20] == 0.0 and not S[[5, 10, 14, 17, 19]].any() and min(S[0], S[6], S[11], S[15], S[18]) > 0.0
        if name in ("one_row_b", "three_rows_b"):
            assert len(o["kept_history"][0]) == 1
        if name == "few_rows_a":
            assert len(f["A"]) < K + 1 and not f["A"][:, 3:].any() and not S.any()
    if name in NOT_REFINED:
        assert o["refined"] == 0 and o["iterations"] == 0 and o["hits"] == 0 and np.array_equal(o["Rt"], f["Rt0"])
    return f


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@functools.lru_cache(maxsize=None)
def tight(name):
    """the room fixture `name` under the reference's commented-out settings -> the oracle's result"""
    f = fixture(name)
    return refine(f["A"], f["B"], f["Rt0"], **io.TIGHT)


def rotation_error(name, o):
    return io.rotation_angle(fixture(name)["true"][:, :3], o["Rt"][:, :3])


@functools.lru_cache(maxsize=None)
def noise():
    """The oracle against itself over the fixtures that take a step, under both settings of the rooms: the kept rows fed to
    the sums in reversed order, and numpy.linalg.lstsq for numpy.linalg.solve -> the largest difference of a pose entry and
    of the rmse."""
    worst = 0.0
    for name, kw, o in [(n, fixture(n)["args"], fixture(n)["oracle"]) for n in NAMES] + \
                       [(n, io.TIGHT, tight(n)) for n in TIGHT_NAMES]:
        if not o["iterations"]:
            continue
        f = fixture(name)
        for variant in (dict(reverse=True), dict(lstsq=True)):
            r = refine(f["A"], f["B"], f["Rt0"], **variant, **kw)
            assert r["iterations"] == o["iterations"] and np.array_equal(r["idx"], o["idx"]), (name, variant)
            worst = max(worst, float(np.abs(r["Rt"] - o["Rt"]).max()), abs(r["rmse"] - o["rmse"]))
    return worst
