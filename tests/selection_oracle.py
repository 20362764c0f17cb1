"""Plain references of the four selection kernel groups whose result is an INDEX -- farthest-point sampling and NMS
(csrc/fps.hip), the SOM front end (csrc/som.hip) and the node KNN (csrc/knn.hip) -- and the inputs their tests share.
numpy and torch on the CPU only; independent of the library (usip_amd is not imported here).

The inputs sit on a lattice: integer and half-integer coordinates make every squared distance exact in float32 and in
float64, so two candidates at the same distance tie EXACTLY, whatever the order of the three squares' sum, and distances
such as 1, 3 and 5 (3-4-5) occur exactly.  The kernels must then return the index the reference's first-occurrence rule
picks, bit for bit.

Every builder returns, next to the data, what the fixture exists for (how many rounds tie, how many of those ties cross
a wave or a slot of the kernel's index layout, how many pairs sit exactly at the radius, ...) and the tests assert these
claims against the floors below, so that an edit of a seed or a size cannot quietly turn a fixture into an easy input.
The floors are about two thirds of what the seeds used by the tests give on the CPU."""
import functools
import math

import numpy as np
import torch

from oracle import detector as od
from oracle import postproc

FPS_T = 1024                   # csrc/fps.hip: point j lives in slot j // 1024 of thread j % 1024; 64 threads to a wave
WAVE = 64


# ----------------------------------------------------------------------------------------------- the lattice
def lattice(n, side, rng, scale=1.0):
    """n points of the side^3 integer lattice times `scale`, float32 [3,n], in shuffled order: without replacement when
    n <= side^3 (all distinct), with replacement otherwise (duplicates)."""
    sites = side ** 3
    flat = rng.permutation(sites)[:n] if n <= sites else rng.integers(0, sites, n)
    xyz = np.stack([flat // (side * side), (flat // side) % side, flat % side]).astype(np.float64) * scale
    out = xyz.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), xyz), "the scaled lattice is not exact in float32"
    return np.ascontiguousarray(out)


# ----------------------------------------------------------------------------------------------- FPS
def fps_with_ties(pts, first, k):
    """oracle.postproc.fps_indices with the rounds counted: pts [n,3] float32 -> (idx i32 [k], dict(tie, wave, slot)):
    the rounds whose maximum is attained by two points or more, those whose tied points sit in two waves or more of the
    kernel's layout, and those whose tied points sit in two slots or more.  The indices are asserted to be
    postproc.fps_indices' own."""
    p = pts.astype(np.float64)
    out = np.zeros(k, np.int32)
    out[0] = first
    dist = ((p[first] - p) ** 2).sum(axis=1)
    tie = wave = slot = 0
    for i in range(1, k):
        tied = np.flatnonzero(dist == dist.max())
        j = int(tied[0])
        out[i] = j
        if len(tied) > 1:
            tie += 1
            wave += len(np.unique((tied % FPS_T) // WAVE)) > 1
            slot += len(np.unique(tied // FPS_T)) > 1
        dist = np.minimum(dist, ((p[j] - p) ** 2).sum(axis=1))
    assert np.array_equal(out, postproc.fps_indices(pts, int(first), k))
    return out, dict(tie=tie, wave=int(wave), slot=int(slot))


def _fps_pack(pts, first, k):
    want, claims = zip(*(fps_with_ties(pts[b].T, int(first[b]), k) for b in range(len(pts))))
    return pts, first, np.stack(want), {key: min(c[key] for c in claims) for key in claims[0]}


@functools.lru_cache(maxsize=None)
def fps_lattice(seed, B, n, side, k, first=None):
    """-> (pts f32 [B,3,n], first i32 [B], want i32 [B,k], claims): claims = the least count over the clouds of tied
    rounds / ties across waves / ties across slots.  first: a tuple, or None for B different random starts."""
    rng = np.random.default_rng(seed)
    pts = np.stack([lattice(n, side, rng) for _ in range(B)])
    if first is None:
        first = rng.permutation(n)[:B] if n >= B else np.zeros(B)
    first = np.asarray(first, np.int32)
    assert first.shape == (B,) and (n < B or len(set(first.tolist())) == B)
    return _fps_pack(pts, first, k)


@functools.lru_cache(maxsize=None)
def fps_repeated(seed, B, distinct, n, k):
    """`distinct` normal points (no two at the same place) repeated to n in shuffled order, every one of them present ->
    (pts, first, want, claims): once the distinct points are used up every running minimum is 0 and numpy's arg-max
    returns index 0; claims adds `used`, the number of leading picks that are distinct points (== distinct, asserted)"""
    rng = np.random.default_rng(seed)
    pts = np.empty((B, 3, n), np.float32)
    for b in range(B):
        base = rng.normal(0, 3, (3, distinct)).astype(np.float32)
        assert len(np.unique(base.T, axis=0)) == distinct
        pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
        pts[b] = base[:, rng.permutation(pick)]
    first = rng.integers(1, n, B).astype(np.int32)
    pts, first, want, claims = _fps_pack(pts, first, k)
    for b in range(B):
        head = pts[b][:, want[b, :distinct]].T
        assert len(np.unique(head, axis=0)) == distinct and not want[b, distinct:].any()
    claims["used"] = distinct
    return pts, first, want, claims


# ----------------------------------------------------------------------------------------------- NMS
def nms_with_ties(kp, sigma, radius):
    """oracle.postproc.nms_order with the picks counted: kp [M,3] f32, sigma [M] f32 -> (kept i32, dict(tie, wave)): the
    picks whose smallest sigma is shared by two live points or more, and those where they sit in two waves or more (one
    thread per point).  The kept indices are asserted to be postproc.nms_order's own."""
    want = postproc.nms_order(kp, sigma, radius)
    alive = np.ones(len(sigma), bool)
    kept, tie, wave = [], 0, 0
    while alive.any():
        live = np.flatnonzero(alive)
        tied = live[sigma[live] == sigma[live].min()]
        m = int(tied[0])
        kept.append(m)
        if len(tied) > 1:
            tie += 1
            wave += len(np.unique(tied // WAVE)) > 1
        d = np.linalg.norm(kp[m:m + 1] - kp, axis=1)
        assert d.dtype == np.float32
        alive &= d > radius
    assert np.array_equal(np.asarray(kept, np.int32), want)
    return want, dict(tie=tie, wave=int(wave))


def pairs_at_radius(kp, radius):
    """kp [M,3] f32 -> the number of ordered pairs (i != j) whose float32 distance EQUALS the radius"""
    d = np.sqrt((((kp[:, None, :] - kp[None, :, :]) ** 2).sum(axis=2)).astype(np.float32))
    assert d.dtype == np.float32
    return int((d == np.float32(radius)).sum())


def nms_reference(kp, sigma, radius):
    """kp [B,3,M], sigma [B,M] -> (order i32 [B,M] zero past the count, count i32 [B], claims): claims = the least count
    over the clouds of tied picks / ties across waves / ordered pairs exactly at the radius, and `kept`, the counts"""
    B, _, M = kp.shape
    order, count = np.zeros((B, M), np.int32), np.zeros(B, np.int32)
    claims = []
    for b in range(B):
        want, c = nms_with_ties(np.ascontiguousarray(kp[b].T), sigma[b], np.float32(radius))
        c["at_radius"] = pairs_at_radius(np.ascontiguousarray(kp[b].T), radius)
        order[b, :len(want)], count[b] = want, len(want)
        claims.append(c)
    out = {key: min(c[key] for c in claims) for key in claims[0]}
    out["kept"] = count.tolist()
    return order, count, out


@functools.lru_cache(maxsize=None)
def nms_lattice(seed, B, M, side, levels=5):
    """-> (kp f32 [B,3,M] on the integer lattice, sigma f32 [B,M] drawn from `levels` values)"""
    rng = np.random.default_rng(seed)
    kp = np.stack([lattice(M, side, rng) for _ in range(B)])
    sigma = (rng.integers(1, levels + 1, (B, M)) * 0.25).astype(np.float32)
    return kp, sigma


# ----------------------------------------------------------------------------------------------- SOM: assignment
def som_assign_f32(x, node):
    """x [B,3,N], node [B,3,M] float32 -> (min_idx i32 [B,N], tied bool [B,N]): float32 d2 = (dx*dx + dy*dy) + dz*dz and
    the FIRST arg-min along the nodes (np.argmin); tied = the minimum is attained by two nodes or more"""
    x, node = np.asarray(x, np.float32), np.asarray(node, np.float32)
    B, _, N = x.shape
    arg, tied = np.empty((B, N), np.int32), np.empty((B, N), bool)
    for b in range(B):
        dx = x[b, 0][:, None] - node[b, 0][None, :]
        dy = x[b, 1][:, None] - node[b, 1][None, :]
        dz = x[b, 2][:, None] - node[b, 2][None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        arg[b] = np.argmin(d2, axis=1)
        tied[b] = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2
    return arg, tied


@functools.lru_cache(maxsize=None)
def som_lattice(seed, B, N, M, side):
    """nodes on the integer lattice, points on the half lattice that covers it -> (x [B,3,N], node [B,3,M], want i32
    [B,N], claims): claims = the least number of points per cloud with two nearest nodes or more"""
    rng = np.random.default_rng(seed)
    node = np.stack([lattice(M, side, rng) for _ in range(B)])
    x = np.stack([lattice(N, 2 * side - 1, rng, 0.5) for _ in range(B)])
    want, tied = som_assign_f32(x, node)
    return x, node, want, dict(tied=int(tied.sum(axis=1).min()))


def som_hand_placed(M, duplicates=False):
    """Nodes on a line, node m at (2m, -1/2, 0), and points at (., 1/2, 0), so d2 = gap^2 + 1 exactly.
    Without duplicates: point n < M-1 sits midway between nodes n and n+1 -- even n: the two nodes of one packed pair; odd
    n: the second of a pair and the first of the next; n = M-2 at odd M: the last pair and the scalar tail -- and must go
    to node n; point M-1+m sits ON node m.
    With duplicates (M >= 7): node 1 is a copy of node 0 (one pair), node 5 of node 2 (two pairs), node M-1 of node 3 (the
    last place, the scalar tail at odd M); the points sit ON the nodes and must go to the first copy.
    -> (x [2,3,N], node [2,3,M], want i32 [2,N], tied bool [2,N]); the second cloud is the first mirrored in x."""
    pos = 2.0 * np.arange(M)
    if duplicates:
        assert M >= 7
        pos[1], pos[5], pos[M - 1] = pos[0], pos[2], pos[3]
        px = pos.copy()
    else:
        px = np.concatenate([pos[:-1] + 1.0, pos])
    gap = np.abs(px[:, None] - pos[None, :])
    want = np.argmin(gap, axis=1).astype(np.int32)                      # 1-D, exact: the first of the nearest nodes
    tied = (gap == gap.min(axis=1, keepdims=True)).sum(axis=1) >= 2
    if duplicates:
        assert want[1] == 0 and want[5] == 2 and want[M - 1] == 3 and tied[[0, 1, 2, 5, 3, M - 1]].all()
    else:
        assert np.array_equal(want, np.concatenate([np.arange(M - 1), np.arange(M)]))
        assert tied[:M - 1].all() and not tied[M - 1:].any()
    x = np.zeros((2, 3, len(px)), np.float32)
    node = np.zeros((2, 3, M), np.float32)
    x[0, 0], node[0, 0] = px, pos
    x[1, 0], node[1, 0] = -px, -pos
    x[:, 1], node[:, 1] = 0.5, -0.5
    return x, node, np.stack([want, want]), np.stack([tied, tied])


# ----------------------------------------------------------------------------------------------- SOM: cluster means
def som_cluster_exact(x, min_idx, M):
    """x [B,3,N] f32, min_idx [B,N] in [0,M) -> (mean f32 [B,3,M], count i32 [B,M], bound f64 [B,3,M]).
    mean = float32(fsum(members)) / (float32(c) + float32(1e-5)), the division in float32: the correctly rounded exact sum
    over the reference's denominator (networks.py:95-96).
    bound: the kernels add the members in double, in some order, c - 1 additions of relative error 2^-53 each on partial
    sums that are at most sum|x|: |sum - exact| <= c 2^-53 sum|x|.  Rounded to float32 and divided by the same
    denominator, the mean is the reference's or its neighbour: |got - want| <= ulp32(want) + c 2^-53 sum|x| / denom."""
    x, min_idx = np.asarray(x, np.float32), np.asarray(min_idx)
    assert min_idx.min() >= 0 and min_idx.max() < M, "an assignment outside the node table"
    B = x.shape[0]
    mean, bound = np.zeros((B, 3, M), np.float32), np.zeros((B, 3, M), np.float64)
    count = np.zeros((B, M), np.int32)
    for b in range(B):
        order = np.argsort(min_idx[b], kind="stable")
        cuts = np.searchsorted(min_idx[b][order], np.arange(M + 1))
        for m in range(M):
            members = order[cuts[m]:cuts[m + 1]]
            c = len(members)
            count[b, m] = c
            denom = np.float32(c) + np.float32(1e-5)
            assert denom.dtype == np.float32
            for ch in range(3):
                v = x[b, ch, members].astype(np.float64)
                mean[b, ch, m] = np.float32(math.fsum(v)) / denom
                bound[b, ch, m] = c * 2.0 ** -53 * float(np.abs(v).sum()) / float(denom)
    bound += np.spacing(np.abs(mean)).astype(np.float64)
    return mean, count, bound


def som_decenter_f32(x, mean, min_idx):
    """float32 x - mean[:, :, min_idx]"""
    centre = np.take_along_axis(mean, np.broadcast_to(np.asarray(min_idx, np.int64)[:, None, :], x.shape), axis=2)
    out = x - centre
    assert out.dtype == np.float32
    return out


CLUSTER_KINDS = ("normal", "cancel", "empty_node", "one_node")


@functools.lru_cache(maxsize=None)
def som_cluster_case(seed, B, N, M, kind):
    """-> (x f32 [B,3,N], min_idx i32 [B,N] from som_assign_f32, claims).
      normal      N(0,1) * 10, nodes drawn from the cloud
      cancel      +-1e4 + N(0,1), the sign drawn per point.  Two points of opposite sign are 3.5e4 apart, so no assignment
                  of THIS cloud puts them into one node; min_idx is the reference assignment of the N(0,1) part alone, which
                  mixes both signs in every node: sum|x| is far above |sum| (claims["cancel"] = the least sum|x| / |sum| over
                  the clouds and coordinates of the largest cluster)
      empty_node  normal, with the last node moved away: nobody is assigned to it (claims["empty"] = its member count, 0)
      one_node    normal, with every node but the last moved away (claims["all"] = 1: the last node holds every point)"""
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1, (B, 3, N))
    if kind == "cancel":
        sign = rng.integers(0, 2, (B, 1, N)) * 2.0 - 1.0
        x, y = (sign * 1e4 + y).astype(np.float32), y.astype(np.float32)
    else:
        x = y = (y * 10).astype(np.float32)
    node = np.stack([y[b][:, rng.permutation(N)[:M]] for b in range(B)]) + np.float32(0.25)
    if kind == "empty_node":
        assert M > 1
        node[:, :, -1] = 1e6
    if kind == "one_node":
        node[:, :, :-1] = 1e6
    min_idx, _ = som_assign_f32(y, node)
    claims = {}
    cnt = np.stack([np.bincount(min_idx[b], minlength=M) for b in range(B)])
    if kind == "cancel":
        worst = np.inf
        for b in range(B):
            v = x[b][:, min_idx[b] == int(np.argmax(cnt[b]))].astype(np.float64)
            worst = min(worst, float((np.abs(v).sum(axis=1) / np.maximum(np.abs(v.sum(axis=1)), 1e-30)).min()))
        claims["cancel"] = worst
    if kind == "empty_node":
        claims["empty"] = int(cnt[:, -1].max())
    if kind == "one_node":
        claims["all"] = int((cnt[:, -1] == N).all())
    return x, min_idx, claims


# ----------------------------------------------------------------------------------------------- KNN
def knn_reference(q, db, K):
    """-> (idx i64 [B,M,K], dist f32 [B,M,N]): od.knn_rows_canonical(od.pairwise_norm(q, db), K) -- nearest first, the
    lower index first on exact ties"""
    dist = od.pairwise_norm(torch.from_numpy(q), torch.from_numpy(db))
    return od.knn_rows_canonical(dist, K).numpy(), dist.numpy()


def knn_tie_claims(dist, K):
    """dist f32 [B,M,N] -> dict(inside, across): the rows with two equal distances among their K smallest, and the rows
    whose K-th and (K+1)-th smallest are equal (the selection itself, not only its order, hangs on the tie-break)"""
    s = np.sort(dist, axis=2)
    inside = (s[:, :, 1:K] == s[:, :, :K - 1]).any(axis=2) if K > 1 else np.zeros(s.shape[:2], bool)
    across = s[:, :, K] == s[:, :, K - 1] if K < s.shape[2] else np.zeros(s.shape[:2], bool)
    return dict(inside=int(inside.sum()), across=int(across.sum()), rows=int(inside.size))


@functools.lru_cache(maxsize=None)
def knn_lattice(seed, B, M, N, side):
    """database on the integer lattice; queries: database points (the first half) and half-lattice points
    -> (q f32 [B,3,M], db f32 [B,3,N], dist f32 [B,M,N])"""
    rng = np.random.default_rng(seed)
    db = np.stack([lattice(N, side, rng) for _ in range(B)])
    own = min(M // 2, N)
    q = np.stack([np.concatenate([db[b][:, rng.permutation(N)[:own]], lattice(M - own, 2 * side - 1, rng, 0.5)], axis=1)
                  for b in range(B)])
    q = np.ascontiguousarray(q)
    return q, db, knn_reference(q, db, 1)[1]


# ----------------------------------------------------------------------------------------------- the cases and their floors
# What the GPU tests run and the CPU test re-derives.  Every floor is about two thirds of what the builder gives at the
# seed written next to it (counted on the CPU, least over the clouds); none of them depends on a kernel's answer.
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))

FPS_CASES = {       # (seed, B, n, side, k, first) -> floors (tied rounds, across waves, across slots)
    "n3000_k200": ((11, 2, 3000, 15, 200, None), (110, 110, 90)),
    "n70_all": ((12, 2, 70, 5, 70, None), (40, 24, 0)),                  # one wave and six lanes
    "n64_all": ((13, 3, 64, 4, 64, None), (38, 0, 0)),                   # one full wave: the whole 4^3 lattice
    "n1_k1": ((14, 2, 1, 1, 1, None), (0, 0, 0)),
    "n1025_all": ((15, 2, 1025, 11, 1025, None), (660, 660, 440)),       # the second slot holds one point, tied with the first
    "n16384_k64": ((16, 2, 16384, 26, 64, None), (15, 14, 14)),          # all 16 slots, at the limit
}

NMS_CASES = {       # (seed, B, M, side, radius) -> floors (ordered pairs at d == r, tied picks, ties across waves)
    "m1024_r1": ((21, 2, 1024, 11, 1.0), (2800, 240, 240)),
    "m1024_below_1": ((21, 2, 1024, 11, BELOW_ONE), (0, 680, 640)),
    "m1000_r5": ((22, 2, 1000, 10, 5.0), (8000, 6, 6)),
    "m65": ((88, 3, 65, 5, 1.0), (90, 16, 0)),                           # one wave and one lane
    "m64": ((87, 2, 64, 5, 1.0), (100, 16, 0)),
    "m1": ((24, 2, 1, 1, 1.0), (0, 0, 0)),
}

SOM_CASES = {       # (seed, B, N, M, side) -> floor (points with two nearest nodes or more)
    "n1001_m33": ((31, 2, 1001, 33, 4), 370),                            # odd M: the scalar tail; N leaves a partial block
    "n1028_m64": ((32, 3, 1028, 64, 4), 540),
    "n2052_m2": ((33, 2, 2052, 2, 2), 440),                              # one packed pair
    "n777_m1": ((34, 2, 777, 1, 3), 0),                                  # the tail alone
    "n300_m5461": ((35, 2, 300, 5461, 18), 160),                         # the node table fills the 64 KiB: 65532 B
}

KNN_SIDES = {64: 4, 256: 7, 257: 7, 512: 9, 513: 9, 1024: 11}           # N -> lattice side (N <= side^3: distinct points)
KNN_M = 70                                                               # 17 full blocks of four queries and a half one


def knn_case(N):
    return knn_lattice(50 + N, 2, KNN_M, N, KNN_SIDES[N])


def knn_floors(N, K):
    """-> (rows with a tie inside their K, rows with a tie across the K-th place), of 140 rows"""
    rows = 2 * KNN_M
    if K == 1:
        return 0, 30
    if K == N:
        return rows, 0
    return rows, 60 if K == 5 else 75


# (N, M): N = 512 the vector tail loop alone, 1024 the unrolled loop alone, 2052 both, 1001 the scalar path; M = 33 and
# M = 1 leave a partial block of four waves
CLUSTER_SHAPES = ((512, 33), (1024, 33), (2052, 33), (1001, 33), (2052, 1), (1001, 1))
CANCEL_FLOOR = 4.0             # least sum|x| / |sum| of the largest cluster of a "cancel" cloud


def cluster_case(N, M, kind):
    return som_cluster_case(40 + N + M, 2, N, M, kind)
