"""numpy / scipy float64 restatement of the reference's MATLAB scan preparation, written from reading it
(evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108, external/findPointNormals.m), plus the two fixed test
inputs of f-7.

Independent of the product: neighbours from scipy's cKDTree (a chunked numpy all-pairs walk when scipy is absent), the
eigenvector from numpy.linalg.eigh -- not the product's Jacobi --, the grid in plain numpy.  Nothing here reads the
reference."""
import numpy as np

try:
    from scipy.spatial import cKDTree
except ImportError:                                        # pragma: no cover
    cKDTree = None


# ------------------------------------------------------------------------------------------------ the two inputs
def scene(seed=7, n=20000):
    """Surface scene: ground, three walls, a sphere and a cylinder with 1 cm noise, shuffled; float32 [n,4]."""
    r = np.random.default_rng(seed)
    parts = []
    m = n // 2
    parts.append(np.stack([r.uniform(-20, 20, m), r.uniform(-20, 20, m), np.full(m, -1.7)], 1))
    m = n // 10
    for s, ax in ((-12, 0), (12, 0), (-15, 1)):
        w = np.stack([r.uniform(-10, 10, m), r.uniform(-10, 10, m), r.uniform(-1.7, 3, m)], 1)
        w[:, ax] = s
        parts.append(w)
    v = r.normal(size=(m, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    parts.append(v * 2.5 + [3, 4, 1])
    m = n - sum(len(p) for p in parts)
    a = r.uniform(0, 2 * np.pi, m)
    parts.append(np.stack([6 + 0.8 * np.cos(a), -5 + 0.8 * np.sin(a), r.uniform(-1.7, 4, m)], 1))
    p = np.concatenate(parts) + r.normal(0, 0.01, (n, 3))
    p = p[r.permutation(n)]
    return np.concatenate([p, r.uniform(0, 0.99, (n, 1))], 1).astype(np.float32)


def ring_scan(seed=3, rings=64, az=1920, max_range=80.0):
    """A 64-ring scan from 1.73 m above a ground plane with 40 boxes; float32 [n,4] (119 768 points at the defaults)."""
    r = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(-24.8, 2.0, rings))
    a = np.linspace(0, 2 * np.pi, az, endpoint=False)
    E, A = np.meshgrid(el, a, indexing="ij")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    t = np.full(len(d), np.inf)
    g = d[:, 2] < 0
    t[g] = -1.73 / d[g, 2]                                   # the ground plane z = -1.73
    nb = 40
    c = np.stack([r.uniform(-70, 70, nb), r.choice([-1, 1], nb) * r.uniform(6, 25, nb), np.zeros(nb)], 1)
    h = np.stack([r.uniform(2, 10, nb), r.uniform(2, 6, nb), r.uniform(1, 8, nb)], 1)
    for ci, hi in zip(c, h):                                 # slab test against each box, nearest entry wins
        lo, up = ci - hi * [1, 1, 0] - [0, 0, 1.73], ci + hi * [1, 1, 1] - [0, 0, 1.73]
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = lo / d, up / d
        tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
        hit = (tn <= tf) & (tn > 0)
        t = np.where(hit & (tn < t), tn, t)
    keep = t < max_range
    t = t[keep] + r.normal(0, 0.02, keep.sum())
    p = d[keep] * t[:, None]
    return np.concatenate([p, r.uniform(0, 0.99, (len(p), 1))], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ neighbours
def neighbours(xyzi, K, workers=1):
    """-> (idx int64 [n,K], d2 float64 [n,K+1]): the K nearest OTHER points (the point left out by index) ascending, and the
    squared distances of the K + 1 nearest others -- column K is the first neighbour NOT taken, for the tie check."""
    p = np.asarray(xyzi, np.float32)[:, :3].astype(np.float64)
    n = len(p)
    if cKDTree is not None:
        _, j = cKDTree(p).query(p, k=min(K + 2, n), workers=workers)
    else:
        j = np.zeros((n, min(K + 2, n)), np.int64)
        for s in range(0, n, 1024):
            d = ((p[s:s + 1024, None, :] - p[None, :, :]) ** 2).sum(-1)
            j[s:s + 1024] = np.argsort(d, axis=1, kind="stable")[:, :j.shape[1]]
    idx = np.zeros((n, K + 1), np.int64)
    d2 = np.full((n, K + 1), np.inf)
    for i in range(n):                                       # "remove self" -- by index, wherever it stands
        row = j[i][j[i] != i][:K + 1]
        idx[i, :len(row)] = row
    valid = min(K + 1, n - 1)
    diff = p[:, None, :] - p[idx[:, :valid]]
    d2[:, :valid] = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    return idx[:, :K], d2


def kth_tie(d2, K, rel=1e-12):
    """points whose K-th and (K+1)-th neighbour distances agree to `rel`: the K-th neighbour is not defined by distance"""
    return np.abs(d2[:, K] - d2[:, K - 1]) <= rel * d2[:, K]


def neighbours_brute(xyzi, K):
    """all pairs with the (d2, index) order spelled out: for the small hand-built cases"""
    p = np.asarray(xyzi, np.float32)[:, :3].astype(np.float64)
    n = len(p)
    out = np.zeros((n, K), np.int64)
    for i in range(n):
        d = p[i] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = [j for j in np.lexsort((np.arange(n), d2)) if j != i]
        out[i] = order[:K]
    return out


# ------------------------------------------------------------------------------------------------ normals
def normals(xyzi, idx, viewpoint=(0.0, 0.0, 1.0)):
    """findPointNormals.m:81-130 with dirLargest = true -> dict(normal [n,3], curvature [n], gap [n] = (l1 - l0) / l2,
    flip [n] = the flip product normal[c] * (p[c] - viewpoint[c]), top2 [n] = difference of the two largest |components|)."""
    p = np.asarray(xyzi, np.float32)[:, :3].astype(np.float64)
    K = idx.shape[1]
    d = p[:, None, :] - p[idx]
    C = np.einsum("nki,nkj->nij", d, d) / K
    w, v = np.linalg.eigh(C)
    nrm = v[:, :, 0].copy()
    tr = w.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        curv = np.where(tr != 0, w[:, 0] / tr, 0.0)
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    nrm[tr == 0] = (0.0, 0.0, 1.0)
    a = np.abs(nrm)
    c = a.argmax(1)                                          # the first of the largest
    rows = np.arange(len(p))
    prod = nrm[rows, c] * (p - np.asarray(viewpoint, np.float64))[rows, c]
    nrm[prod > 0] *= -1.0
    s = np.sort(a, axis=1)
    return dict(normal=nrm, curvature=curv, gap=gap, flip=prod, top2=s[:, 2] - s[:, 1])


def comparable(o, gap=1e-3, flip=1e-9, top2=1e-9):
    """the points whose normal is defined well enough to compare: the leave-out rule of the f-7 tests"""
    return (o["gap"] >= gap) & (np.abs(o["flip"]) >= flip) & (o["top2"] >= top2)


# ------------------------------------------------------------------------------------------------ grid
def grid(xyzi, nrm64, leaf=0.2):
    """The project's 'gridAverage': -> dict(keys [m], members: list of index arrays (ascending), rows float32 [m,8])."""
    a = np.asarray(xyzi, np.float32)
    p = a[:, :3].astype(np.float64)
    lo = a[:, :3].min(0).astype(np.float64)
    hi = a[:, :3].max(0).astype(np.float64)
    cell = np.floor((p - lo) / leaf).astype(np.int64)
    dims = np.floor((hi - lo) / leaf).astype(np.int64) + 1
    key = (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0]
    keys, inv = np.unique(key, return_inverse=True)
    m = len(keys)
    order = np.argsort(inv, kind="stable")
    bounds = np.concatenate(([0], np.cumsum(np.bincount(inv, minlength=m))))
    members = [order[bounds[c]:bounds[c + 1]] for c in range(m)]
    cnt = np.bincount(inv, minlength=m).astype(np.float64)
    vals = np.concatenate((p, np.asarray(nrm64, np.float64), a[:, 3:4].astype(np.float64)), 1)     # x y z nx ny nz c r
    mean = np.stack([np.bincount(inv, weights=vals[:, k], minlength=m) for k in range(8)], 1) / cnt[:, None]
    nm = mean[:, 3:6]
    ln = np.sqrt((nm * nm).sum(1))
    first = np.asarray(nrm64, np.float64)[[mem[0] for mem in members], :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        nm = np.where(ln[:, None] == 0, first, nm / ln[:, None])
    rows = np.concatenate((mean[:, :3], nm, mean[:, 6:8]), 1).astype(np.float32)
    return dict(keys=keys, members=members, rows=rows, normal_len=ln)


def ulp_apart(a, b):
    """distance of two float32 arrays in units of the float32 spacing at the larger magnitude"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp
