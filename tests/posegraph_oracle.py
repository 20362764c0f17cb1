"""A numpy restatement of the f-14 contract (include/usip_hip.h): the dense information matrix over aligned points and the
two-stage robust pose-graph optimisation.  It shares no code with the library: a loop over edges, 4 x 4 matrices, numpy.linalg
for the factorisation and the solve, numpy.sin / numpy.cos for the step's rotation, numpy.add.at for the information.  The
scene generator and the fixtures of tests/test_posegraph_cpu.py and tests/test_posegraph_gpu.py live here too."""
import numpy as np

S6 = np.diag([1.0, 1.0, 1.0, 0.5, 0.5, 0.5])


def to4(Rt):
    return np.vstack((np.asarray(Rt, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]))


def rigid_inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def quat_vector(R):
    """Shepperd: the largest of (trace, R00, R11, R22), the lowest index on ties; w >= 0."""
    c = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]
    b = int(np.argmax(c))                                           # argmax returns the first of equal values
    if b == 0:
        s = np.sqrt(1.0 + c[0])
        w, v = 0.5 * s, np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (0.5 / s)
    elif b == 1:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        w, v = (R[2, 1] - R[1, 2]) * (0.5 / s), np.array([0.5 * s, (R[0, 1] + R[1, 0]) * (0.5 / s), (R[0, 2] + R[2, 0]) * (0.5 / s)])
    elif b == 2:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        w, v = (R[0, 2] - R[2, 0]) * (0.5 / s), np.array([(R[0, 1] + R[1, 0]) * (0.5 / s), 0.5 * s, (R[1, 2] + R[2, 1]) * (0.5 / s)])
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        w, v = (R[1, 0] - R[0, 1]) * (0.5 / s), np.array([(R[0, 2] + R[2, 0]) * (0.5 / s), (R[1, 2] + R[2, 1]) * (0.5 / s), 0.5 * s])
    return (-v if w < 0 else v), b, w < 0


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def adjoint(E):
    R, t = E[:3, :3], E[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3], Ad[3:, 3:], Ad[:3, 3:] = R, R, skew(t) @ R
    return Ad


def rot_zyx(phi):
    c, s = np.cos(phi), np.sin(phi)
    Rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    Ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    Rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1.0]])
    return Rz @ Ry @ Rx


def edge_terms(T, i, j, X, L, tau2):
    E = rigid_inv(T[i]) @ T[j]
    D = E @ rigid_inv(X)
    e = np.concatenate((D[:3, 3], quat_vector(D[:3, :3])[0]))
    f = float(e @ (L @ e))
    if j == i + 1:
        return E, e, f, 1.0
    mu = L[0, 0] * tau2
    den = mu + f
    return E, e, f, ((mu / den) ** 2 if np.isfinite(den) and den > 0 else 0.0)


def weights(T, edges, X, L, tau2, kept=None):
    w, f = np.zeros(len(edges)), np.zeros(len(edges))
    for k, (i, j) in enumerate(edges):
        _, _, f[k], w[k] = edge_terms(T, i, j, X[k], L[k], tau2)
        if kept is not None and j != i + 1 and not kept[k]:
            w[k] = 0.0
    return w, f


def optimise(n, edges, X, L, T0, tau2=0.04, prune=0.25, iterations1=32, iterations2=32, descending=False):
    """-> dict(T [n,3,4], weight1, weight2, energy, kept, iterations_done [2], last_step [2], status).  descending: the
    unknowns enter the linear system in descending fragment order -- the same mathematics, other rounding."""
    X4, T = [to4(x) for x in X], [to4(t) for t in T0]
    M = 6 * (n - 1)
    order = np.arange(n - 1)[::-1] if descending else np.arange(n - 1)           # block -> fragment - 1
    where = np.empty(n - 1, np.int64)
    where[order] = np.arange(n - 1)
    sl = lambda a: slice(6 * where[a - 1], 6 * where[a - 1] + 6)
    status, done, last, kept, w1 = 0, [0, 0], [0.0, 0.0], None, None
    for stage in range(2):
        for it in range(iterations1 if stage == 0 else iterations2):
            if status:
                break
            H, g = np.zeros((M, M)), np.zeros(M)
            for k, (i, j) in enumerate(edges):
                E, e, f, l = edge_terms(T, i, j, X4[k], L[k], tau2)
                if stage == 1 and j != i + 1 and not kept[k]:
                    l = 0.0
                if not l > 0:
                    continue
                Ji, Jj = -S6, S6 @ adjoint(E)
                W = l * L[k]
                H[sl(j), sl(j)] += Jj.T @ W @ Jj
                g[sl(j)] += Jj.T @ W @ e
                if i >= 1:
                    H[sl(i), sl(i)] += Ji.T @ W @ Ji
                    g[sl(i)] += Ji.T @ W @ e
                    H[sl(j), sl(i)] += Jj.T @ W @ Ji
                    H[sl(i), sl(j)] += Ji.T @ W @ Jj
            with np.errstate(all="ignore"):
                try:
                    if not np.all(np.isfinite(H)):
                        raise np.linalg.LinAlgError
                    C = np.linalg.cholesky(H)
                    d = -np.linalg.solve(C.T, np.linalg.solve(C, g))
                except np.linalg.LinAlgError:
                    status = 1
                    break
            if not np.all(np.isfinite(d)):
                status = 2
                break
            d = np.stack([d[sl(a)] for a in range(1, n)])
            if np.any(np.abs(d[:, 3:]) > np.pi):
                status = 3
                break
            for a in range(1, n):
                step = np.eye(4)
                step[:3, :3], step[:3, 3] = rot_zyx(d[a - 1, 3:]), d[a - 1, :3]
                T[a] = T[a] @ step
            done[stage], last[stage] = it + 1, float(np.max(np.abs(d)))
        w, f = weights(T, edges, X4, L, tau2, kept if stage == 1 else None)
        if stage == 0:
            w1 = w
            kept = np.array([j == i + 1 or w[k] >= prune for k, (i, j) in enumerate(edges)], bool)
    return dict(T=np.stack([t[:3] for t in T]), weight1=w1, weight2=w, energy=f, kept=kept.astype(np.uint8),
                iterations_done=np.array(done, np.int32), last_step=np.array(last), status=status)


# ------------------------------------------------------------------------------------------------ the information matrix
def information(rows1, idx, d2, radius, reverse=False):
    """sum of A'A at rows1[idx[i]] over the rows with sqrt(d2) < radius, with multiplicity (numpy.add.at) -> (6 x 6, count)"""
    hit = np.nonzero(np.sqrt(np.asarray(d2, np.float64)) < radius)[0]
    if reverse:
        hit = hit[::-1]
    s = np.asarray(rows1, np.float64)[np.asarray(idx)[hit], :3]
    A = np.zeros((len(hit), 3, 6))
    A[:, 0, 0] = A[:, 1, 1] = A[:, 2, 2] = 1.0
    A[:, 0, 4], A[:, 0, 5] = 2 * s[:, 2], -2 * s[:, 1]
    A[:, 1, 3], A[:, 1, 5] = -2 * s[:, 2], 2 * s[:, 0]
    A[:, 2, 3], A[:, 2, 4] = 2 * s[:, 1], -2 * s[:, 0]
    out = np.zeros((1, 6, 6))
    np.add.at(out, np.zeros(len(hit), np.int64), np.einsum("nki,nkj->nij", A, A))
    return out[0], len(hit)


def points_information(points):
    s = np.asarray(points, np.float64)
    return information(s, np.arange(len(s)), np.zeros(len(s)), 1.0)[0]


# ------------------------------------------------------------------------------------------------ scenes
def rotvec(v):
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    K = skew(v / a)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def disturb(rng, rot, trans):
    T = np.eye(4)
    axis = rng.normal(size=3)
    T[:3, :3] = rotvec(axis / np.linalg.norm(axis) * rot)
    d = rng.normal(size=3)
    T[:3, 3] = d / np.linalg.norm(d) * trans
    return T


def make_scene(seed, n, true_loops, false_loops, noise=0.003):
    """A chain of random poses (sigma 0.3 rad, 0.6 m per step), an edge's information from 200-2000 random points in a 3 m
    cube, edge noise 0.003 (rad and m), false loops composed with a (0.8 rad, 1.0 m) disturbance.  -> dict(n, edges, X, L,
    T0, truth u8 [E]: 1 for the edges that must be kept)."""
    rng = np.random.default_rng(seed)
    poses = [np.eye(4)]
    for _ in range(n - 1):
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = rotvec(rng.normal(size=3) * 0.3), rng.normal(size=3) * 0.6
        poses.append(poses[-1] @ step)
    loops = [(i, j) for i in range(n) for j in range(i + 2, n)]
    rng.shuffle(loops)
    assert true_loops + false_loops <= len(loops)
    chosen = {p: True for p in loops[:true_loops]}
    chosen.update({p: False for p in loops[true_loops:true_loops + false_loops]})
    chosen.update({(k, k + 1): True for k in range(n - 1)})
    edges = sorted(chosen)
    X, L = [], []
    for i, j in edges:
        rel = rigid_inv(poses[i]) @ poses[j]
        jitter = np.eye(4)
        jitter[:3, :3], jitter[:3, 3] = rotvec(rng.normal(size=3) * noise), rng.normal(size=3) * noise
        rel = rel @ jitter
        if not chosen[(i, j)]:
            rel = rel @ disturb(rng, 0.8, 1.0)
        X.append(rel[:3])
        L.append(points_information(rng.uniform(-1.5, 1.5, size=(int(rng.integers(200, 2001)), 3))))
    X, L = np.stack(X), np.stack(L)
    return finish(n, edges, X, L, np.array([chosen[e] for e in edges], np.uint8))


def finish(n, edges, X, L, truth):
    T0 = [np.eye(4)]
    where = {e: k for k, e in enumerate(edges)}
    for k in range(n - 1):
        T0.append(T0[-1] @ to4(X[where[(k, k + 1)]]) if (k, k + 1) in where else T0[-1])
    return dict(n=n, edges=list(edges), X=np.ascontiguousarray(X), L=np.ascontiguousarray(L),
                T0=np.stack([t[:3] for t in T0]), truth=np.asarray(truth, np.uint8))


EXACT = {"half_x": np.diag([1.0, -1.0, -1.0]), "half_y": np.diag([-1.0, 1.0, -1.0]), "half_z": np.diag([-1.0, -1.0, 1.0]),
         "third_111": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])}


def exact_scene(name, seed=5):
    """Four fragments in a row, one true loop (0, 2), and a false loop (0, 3) whose transform is the truth followed by a
    turn with exact entries: a half turn about x, y or z (the quaternion's three other branches) or 120 degrees about (1, 1, 1)."""
    sc = make_scene(seed, 4, 1, 0)
    edges = sorted(set(sc["edges"]) | {(0, 3)})
    where = {e: k for k, e in enumerate(sc["edges"])}
    rng = np.random.default_rng(seed + 1)
    X, L, truth = [], [], []
    for e in edges:
        if e in where:
            X.append(sc["X"][where[e]])
            L.append(sc["L"][where[e]])
            truth.append(1)
        else:
            rel = np.eye(4)
            for k in range(3):
                rel = rel @ to4(sc["X"][where[(k, k + 1)]])
            turn = np.eye(4)
            turn[:3, :3] = EXACT[name]
            X.append((rel @ turn)[:3])
            L.append(points_information(rng.uniform(-1.5, 1.5, size=(500, 3))))
            truth.append(0)
    return finish(4, edges, np.stack(X), np.stack(L), truth)


def zero_information_scene(seed=9):
    """4 / 2 / 1 with the information of one true loop set to zero: its weight is 0 and it is dropped."""
    sc = make_scene(seed, 4, 2, 1)
    k = [k for k, (i, j) in enumerate(sc["edges"]) if j - i > 1 and sc["truth"][k]][0]
    sc["L"][k] = 0.0
    sc["truth"][k] = 0
    return sc


SCENES = {"2/0/0": lambda: make_scene(1, 2, 0, 0), "3/1/0": lambda: make_scene(2, 3, 1, 0),
          "4/2/1": lambda: make_scene(3, 4, 2, 1), "12/14/8": lambda: make_scene(4, 12, 14, 8),
          "43/60/15": lambda: make_scene(5, 43, 60, 15), "44/60/15": lambda: make_scene(6, 44, 60, 15),
          "57/200/30": lambda: make_scene(7, 57, 200, 30),
          "half_x": lambda: exact_scene("half_x"), "half_y": lambda: exact_scene("half_y"),
          "half_z": lambda: exact_scene("half_z"), "third_111": lambda: exact_scene("third_111"),
          "zero_information": zero_information_scene}
ITERATIONS = {"2/0/0": (4, 4), "3/1/0": (8, 4), "4/2/1": (12, 4), "12/14/8": (12, 4), "43/60/15": (10, 3), "44/60/15": (10, 3),
              "57/200/30": (10, 3), "half_x": (12, 4), "half_y": (12, 4), "half_z": (12, 4), "third_111": (12, 4),
              "zero_information": (12, 4), "stage2_of_0": (12, 0)}
SCENES["stage2_of_0"] = lambda: make_scene(3, 4, 2, 1)


def batch_of(scenes):
    """The padded arrays the library takes (what usip_amd.posegraph.pack_graphs builds), from scenes of this module."""
    S, Nmax, Emax = len(scenes), max(max(sc["n"] for sc in scenes), 2), max(max(len(sc["edges"]) for sc in scenes), 1)
    b = {"n": np.array([sc["n"] for sc in scenes], np.int32), "ecount": np.array([len(sc["edges"]) for sc in scenes], np.int32),
         "edge_i": np.zeros((S, Emax), np.int32), "edge_j": np.zeros((S, Emax), np.int32), "X": np.zeros((S, Emax, 3, 4)),
         "info": np.zeros((S, Emax, 6, 6)), "T0": np.zeros((S, Nmax, 3, 4))}
    for s, sc in enumerate(scenes):
        E = len(sc["edges"])
        if E:
            b["edge_i"][s, :E], b["edge_j"][s, :E] = np.array(sc["edges"], np.int32).T
            b["X"][s, :E], b["info"][s, :E] = sc["X"], sc["L"]
        b["T0"][s, :sc["n"]] = sc["T0"]
    return b


# ------------------------------------------------------------------------------------------------ information fixtures
def information_bank(seed=11):
    """-> (clouds, pairs): clouds of 0, 1, 40, 255, 256, 257 and 515 rows, and a lattice of integers / 64; pairs (frag1,
    frag2) whose fragment 2 has each of those lengths, with ids outside the bank among them."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 40, 255, 256, 257, 515]
    clouds = [rng.uniform(-0.5, 0.5, size=(m, 3)).astype(np.float32) for m in sizes]
    g = np.arange(-4, 5) / 64.0
    clouds.append(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32))      # 729 rows
    # probes outside the lattice along x, at exactly 2 / 64, 3 / 64 and 4 / 64 from its face (every value exact in float32)
    clouds.append(np.array([[(4 + m) / 64.0, y / 64.0, z / 64.0] for m in (2, 3, 4) for y in (-4, 0, 3) for z in (-2, 0, 4)],
                           np.float32))
    # fragment 2 of 1, 255, 256, 257 and 515 queries; every query on the one row of fragment 1; empty fragments; the lattice
    # with itself; ids outside the bank (clamped)
    pairs = [(6, 1), (6, 3), (6, 4), (6, 5), (5, 6), (1, 6), (2, 6), (6, 0), (0, 6), (7, 7), (3, 3), (-1, 6), (6, 12), (4, 2),
             (7, 8)]
    return clouds, pairs


LATTICE_PAIR, LATTICE_RADIUS, LATTICE_COUNT = 14, 3.0 / 64.0, 9       # strict: the probes at exactly 3 / 64 do not count
