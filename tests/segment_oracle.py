"""Plain references of the reduce-by-destination kernels (csrc/segment.hip, csrc/knn_layer.hip, the values side of
csrc/index_max.hip) and of the element-wise tail (csrc/head.hip), and the inputs their tests share.  numpy on the CPU only;
independent of the library (usip_amd is not imported here).

The inputs are dyadic, so that every product and every fused multiply-add of a kernel is exact in float32: each reference
redoes the arithmetic in float64 and ASSERTS that the float32 value it returns is that number (exact()).
  KNN first layer, forward   database, query  multiples of 2^-2 within +-2       d = db - q: a 2^-2, |a| <= 16
                             W                multiples of 2^-2 within +-1       w d: b 2^-4, |b| <= 64; three of them <= 192
                             U                multiples of 2^-4 within +-2       y = U + t: c 2^-4, |c| <= 224; y^2 <= 50176 2^-8
  KNN first layer, backward  Y, dZ            multiples of 2^-4 within +-8 / +-4
                             a1, q1           multiples of 2^-2 within +-2 / +-1; a0 2^-4 within +-4, q0 2^-6 within +-1
                             fma(y, a1, a0), fma(q1, y, q0), g = fma(a1, dyh, .): multiples of 2^-6 below 2^11 units
                             dcoord           multiples of 2^-2 within +-4       g d: 2^-8, below 2^15 units
  node-max                   data multiples of 2^-4 within +-8 (and -2000, NaN where a case says so); gradients 2^-4 within +-8
A reduction whose tree the oracle does not restate (the forward's sum / sum^2, dWc, position 0 of the node-max backwards) is
"exact in any order" when the sum of the |terms| stays below 2^24 units of the terms' step: any_order_exact() decides it from
the data, and where it does not hold, rounding_bound() counts roundings along the kernel's longest addition chain.

The segment sums need no such thing: given the device's own `perm`, segment_sum_listorder() follows the kernel's chain
(((0 + r0) + r1) + r2) + ... in float32 (np.cumsum with dtype float32 is sequential: test_segment_oracle_cpu.py pins it),
so it holds for ANY float inputs.

Every builder returns, next to its data, the claims the fixture exists for; test_segment_oracle_cpu.py asserts them against
the floors written here (none depends on a kernel's answer)."""
import functools
import math

import numpy as np

FLOOR = np.float32(-1000.0)                       # index_max: a maximum must be strictly above it


def dyadic(rng, shape, log2_step, bound):
    """float32 multiples of 2^-log2_step within +-bound, asserted exact; never -0.0"""
    n = int(bound * (1 << log2_step))
    v = rng.integers(-n, n + 1, shape).astype(np.float64) / float(1 << log2_step)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exact(v64, what):
    """the float32 of a float64 result, asserted to be that number (nothing rounded); -0.0 becomes +0.0 nowhere here"""
    out = np.asarray(v64, np.float64).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v64, equal_nan=True), "%s is not exact in float32" % what
    return out


def any_order_exact(terms64, log2_step):
    """terms64 [..., T] (multiples of 2^-log2_step): True where sum |terms| < 2^24 units, so that every partial sum in every
    order is a float32"""
    units = np.abs(np.asarray(terms64, np.float64)) * float(1 << log2_step)
    assert np.array_equal(units, np.round(units)), "a term is no multiple of the step"
    return units.sum(axis=-1) < float(1 << 24)


def rounding_bound(terms64, chain):
    """(chain + 2) 2^-24 sum |terms|: `chain` additions on the longest path, each rounding by at most 2^-24 of a partial sum
    that is at most sum |terms|; + 2 for the float32 of the terms themselves and of the reference"""
    return (chain + 2) * 2.0 ** -24 * np.abs(np.asarray(terms64, np.float64)).sum(axis=-1)


# ----------------------------------------------------------------------------------------------- CSR
def csr_start(idx, N):
    """idx i32 [B,P] -> start i32 [B,N+1]: the cumulative bincount of the entries in [0, N)"""
    idx = np.asarray(idx)
    B = idx.shape[0]
    start = np.zeros((B, N + 1), np.int32)
    for b in range(B):
        ok = idx[b][(idx[b] >= 0) & (idx[b] < N)]
        start[b, 1:] = np.cumsum(np.bincount(ok, minlength=N))
    return start


def check_perm(idx, N, start, perm):
    """Every cloud, every cell: start is csr_start; the members of each segment are exactly the positions that name the
    cell (out-of-range entries appear nowhere); inside a segment the 64-position block p // 64 never decreases (the kernel
    hands slots out wave slice by wave slice and, inside one, 64 positions at a time; the order INSIDE a block is the
    hardware's).  -> the number of segments checked; raises AssertionError"""
    idx, start, perm = np.asarray(idx), np.asarray(start), np.asarray(perm)
    B, P = idx.shape
    assert start.shape == (B, N + 1) and perm.shape == (B, P)
    assert np.array_equal(start, csr_start(idx, N)), "start is not the cumulative bincount"
    for b in range(B):
        total = int(start[b, N])
        seg = perm[b, :total].astype(np.int64)
        assert total == 0 or (seg.min() >= 0 and seg.max() < P), "cloud %d: a position outside [0, P)" % b
        cell = np.repeat(np.arange(N), np.diff(start[b]))
        assert np.array_equal(idx[b][seg], cell), "cloud %d: a position in the segment of another cell" % b
        valid = np.flatnonzero((idx[b] >= 0) & (idx[b] < N))
        want = valid[np.argsort(idx[b][valid], kind="stable")]             # by cell, ascending p inside
        assert np.array_equal(seg[np.lexsort((seg, cell))], want), "cloud %d: a segment is not its cell's positions" % b
        same = cell[1:] == cell[:-1]
        assert (np.diff(seg // 64)[same] >= 0).all(), "cloud %d: a 64-position block behind a later one" % b
    return B * N


def idx_of_lengths(rng, lengths, N, P, junk=0):
    """i32 [P]: cell n named lengths[n] times (cells past len(lengths): the rest, spread at random over them; none if there
    are none), `junk` entries out of range (negative and >= N in turn), in random order"""
    lengths = list(lengths)
    rest = P - junk - sum(lengths)
    assert rest >= 0 and len(lengths) <= N and (rest == 0 or len(lengths) < N)
    parts = [np.full(l, n) for n, l in enumerate(lengths)]
    parts.append(rng.integers(len(lengths), N, rest) if rest else np.zeros(0, np.int64))
    parts.append(np.asarray([(-1 - i) if i % 2 == 0 else (N + i) for i in range(junk)], np.int64))
    out = np.concatenate(parts).astype(np.int32)
    rng.shuffle(out)
    return out


def segment_claims(idx, N):
    """-> dict: empty (cells nobody names, least over the clouds), longest (the longest segment), junk (out-of-range
    entries), lengths (the set of segment lengths that occur)"""
    idx = np.asarray(idx)
    counts = np.stack([np.bincount(r[(r >= 0) & (r < N)], minlength=N) for r in idx]) if idx.shape[0] else np.zeros((0, N), int)
    return dict(empty=int((counts == 0).sum(axis=1).min()) if counts.size else N,
                longest=int(counts.max()) if counts.size else 0,
                junk=int(((idx < 0) | (idx >= N)).sum()), lengths=set(np.unique(counts).tolist()))


# ----------------------------------------------------------------------------------------------- segment sums
def segment_sum_listorder(src, start, perm, C, coff=0):
    """dx[b,c,n] = (((0 + r[p0]) + r[p1]) + ...) in float32 over perm[b, start[b,n] : start[b,n+1]], r = src[b, coff + c]
    -- the kernel's chain, for any float inputs.  src [B,Ctot,P] -> f32 [B,C,N]"""
    src, start, perm = np.asarray(src, np.float32), np.asarray(start), np.asarray(perm)
    B, N = start.shape[0], start.shape[1] - 1
    dx = np.zeros((B, C, N), np.float32)
    zero = np.zeros((C, 1), np.float32)
    for b in range(B):
        rows = src[b, coff:coff + C]
        for n in range(N):
            s0, s1 = int(start[b, n]), int(start[b, n + 1])
            if s1 > s0:
                chain = np.concatenate([zero, rows[:, perm[b, s0:s1]]], axis=1)
                dx[b, :, n] = np.cumsum(chain, axis=1, dtype=np.float32)[:, -1]
    return dx


def segment_sum64(src, idx, C, N, coff=0):
    """the same sums in float64 by np.add.at over idx (no perm needed) -> f64 [B,C,N]"""
    src, idx = np.asarray(src, np.float64), np.asarray(idx)
    B = src.shape[0]
    dx = np.zeros((B, C, N), np.float64)
    for b in range(B):
        ok = np.flatnonzero((idx[b] >= 0) & (idx[b] < N))
        for c in range(C):
            np.add.at(dx[b, c], idx[b][ok], src[b, coff + c][ok])
    return dx


# ----------------------------------------------------------------------------------------------- KNN first layer
def knn_forward(U, W, database, query, idx):
    """Y[b,c,p] = U[b,c,n] + fma(wz, dz, fma(wy, dy, wx dx)), d = database[b,:,n] - query[b,:,m] (ONE float32 subtraction),
    n = clamp(idx[b,m,k], 0, N - 1), p = m K + k; W [Cout, >= 3] (columns 0..2 are read).  Every step asserted exact.
    -> (Y f32 [B,Cout,P], d f32 [B,3,P], n i64 [B,P])"""
    U, W = np.asarray(U, np.float32), np.asarray(W, np.float32)
    database, query, idx = np.asarray(database, np.float32), np.asarray(query, np.float32), np.asarray(idx)
    B, Cout, N = U.shape
    _, M, K = idx.shape
    n = np.clip(idx.astype(np.int64), 0, N - 1).reshape(B, M * K)
    m = np.arange(M * K) // K
    d = np.take_along_axis(database, np.broadcast_to(n[:, None, :], (B, 3, M * K)), axis=2) - query[:, :, m]
    assert d.dtype == np.float32
    d64, w64 = d.astype(np.float64), W.astype(np.float64)
    t = exact(w64[None, :, 0, None] * d64[:, None, 0], "wx dx")
    t = exact(w64[None, :, 1, None] * d64[:, None, 1] + t, "fma(wy, dy, .)")
    t = exact(w64[None, :, 2, None] * d64[:, None, 2] + t, "fma(wz, dz, .)")
    u = np.take_along_axis(U, np.broadcast_to(n[:, None, :], (B, Cout, M * K)), axis=2)
    return exact(u.astype(np.float64) + t, "U + t"), d, n


def knn_stats(Y):
    """-> (terms64 [2,Cout,B,P]: y and y^2 per cloud, the layout [2][Cout][B] of the kernel's partials on the leading axes)"""
    y = np.asarray(Y, np.float64).transpose(1, 0, 2)
    return np.stack([y, y * y])


def knn_backward_g(dZ, Y, coef4, relu):
    """g = fma(a1, relu ? (fma(y, a1, a0) > 0 ? dz : 0) : dz, fma(q1, y, q0)), coef4 [4,Cout] = (a1, a0, q1, q0); asserted
    exact -> f32 [B,Cout,P]"""
    y, dz, c = np.asarray(Y, np.float64), np.asarray(dZ, np.float64), np.asarray(coef4, np.float64)[:, None, :, None]
    z = exact(y * c[0] + c[1], "fma(y, a1, a0)")
    dyh = np.where(z > 0, dz, 0.0) if relu else dz
    inner = exact(c[2] * y + c[3], "fma(q1, y, q0)")
    return exact(c[0] * dyh + inner, "g")


def knn_dwc_terms(g, dcoord):
    """-> terms64 [Cout,3,B*P]: g[b,c,p] d[b,j,p]; dWc[c,j] is their sum"""
    g, d = np.asarray(g, np.float64), np.asarray(dcoord, np.float64)
    t = g[:, :, None, :] * d[:, None, :, :]                                 # [B,Cout,3,P]
    exact(t, "g d")
    return t.transpose(1, 2, 0, 3).reshape(t.shape[1], 3, -1)


# (seed, B, Cout, N, M, K, the lengths of the first cells' lists or None for random indices)
#   first-destination lists of 0, 1, 31, 32, 33, 35, 36, 37: the 32 prefetched entries alone, the hand-over to the
#   4-unrolled walk (36: exactly one trip; 37: a trip and the tail; 33, 35: the tail alone)
HANDOVER = (0, 1, 31, 32, 33, 35, 36, 37)
KNN_CASES = {
    "p4": (1, 2, 4, 2, 1, 4, None),
    "handover": (2, 2, 4, 40, 64, 8, HANDOVER),                             # P = 512, 205 in the named lists
    "handover_odd": (3, 2, 3, 40, 64, 8, HANDOVER),                         # odd Cout: the one-row form by itself
    "one_list": (4, 1, 2, 5, 16, 8, (0, 128)),                              # cell 1 holds all of P = 128
    "n513": (5, 1, 2, 513, 130, 8, None),                                   # P = 1040: destinations 512 (two rows), 256.. (one row) past NT
    "n1489": (6, 1, 2, 1489, 375, 8, None),                                 # P = 3000: the forward's LDS limit
    "cout1": (7, 2, 1, 33, 8, 4, None),
    "cout9": (8, 2, 9, 33, 255, 4, None),                                   # P = 1020
    "cout7_p1028": (9, 1, 7, 33, 257, 4, None),                             # a second, partly filled trip of the 4 x 256 unroll
    "cout8_p1024": (10, 1, 8, 33, 256, 4, None),
    "k1": (11, 2, 2, 1, 8, 1, None),                                        # N = 1, K = 1
    "p4100": (12, 1, 2, 64, 1025, 4, None),                                 # ends inside the 2nd NT*4*UN trip of the one-row form
    "p8196": (13, 1, 2, 64, 2049, 4, None),                                 # two rows no longer fit: <1,256> by size
    "p16384": (14, 1, 2, 1489, 1024, 16, None),
    "p16384_odd": (15, 2, 3, 64, 1024, 16, None),
    # the backward's channel-chunk loop on a 256-CU device: B Cout / 2 two-row chunks, tpw of them per workgroup
    "chunk2048": (16, 64, 32, 2, 1, 4, None),                               # tpw 2
    "chunk4096": (17, 64, 64, 2, 1, 4, None),                               # tpw 4
    "chunk8320": (18, 64, 130, 2, 1, 4, None),                              # tpw 8, ragged: 65 chunks over 9 workgroups
}
CHUNK_TPW = {"chunk2048": 2, "chunk4096": 4, "chunk8320": 8}


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """-> dict(U, W, database, query, idx, dZ, Yb, coef4, claims).  idx holds clamped entries (-3 and N + 5) where the lists
    are random; Yb / dZ / coef4 are the backward's own dyadic inputs.  claims: segment_claims of the clamped indices, plus
    zero_act (positions where fma(y, a1, a0) is exactly 0: ReLU's `> 0` against `>= 0`) and neg_act"""
    seed, B, Cout, N, M, K, lengths = KNN_CASES[name]
    rng = np.random.default_rng(9000 + seed)
    P = M * K
    if lengths is None:
        idx = rng.integers(0, N, (B, P)).astype(np.int32)
        if P >= 8:
            idx[:, 1], idx[:, P - 2] = -3, N + 5
    else:
        idx = np.stack([idx_of_lengths(rng, lengths, N, P) for _ in range(B)])
    c = dict(U=dyadic(rng, (B, Cout, N), 4, 2), W=dyadic(rng, (Cout, 5), 2, 1), database=dyadic(rng, (B, 3, N), 2, 2),
             query=dyadic(rng, (B, 3, M), 2, 2), idx=idx.reshape(B, M, K),
             dZ=dyadic(rng, (B, Cout, P), 4, 4), Yb=dyadic(rng, (B, Cout, P), 4, 8),
             coef4=np.stack([dyadic(rng, Cout, 2, 2), dyadic(rng, Cout, 4, 4), dyadic(rng, Cout, 2, 1), dyadic(rng, Cout, 6, 1)]))
    c["coef4"][0][c["coef4"][0] == 0] = np.float32(0.75)                    # a1 = 0 would hide dyh
    z = c["Yb"].astype(np.float64) * c["coef4"][0].astype(np.float64)[None, :, None] + c["coef4"][1].astype(np.float64)[None, :, None]
    c["claims"] = dict(segment_claims(np.clip(idx, 0, N - 1), N), zero_act=int((z == 0).sum()), neg_act=int((z < 0).sum()),
                       clamped=int(((idx < 0) | (idx >= N)).sum()))
    return c


# ----------------------------------------------------------------------------------------------- node-max values
def index_max(data, index, K, C=None):
    """-> i32 [B,C,K]: per (b, c, k) the LOWEST n with index[b,n] == k whose value is the maximum over those n, if that
    maximum is strictly above -1000 (a NaN is above nothing); else 0"""
    data, index = np.asarray(data, np.float32), np.asarray(index)
    B, Ctot, N = data.shape
    C = Ctot if C is None else C
    out = np.zeros((B, C, K), np.int32)
    for b in range(B):
        order = np.argsort(index[b], kind="stable")
        ks, first = np.unique(index[b][order], return_index=True)
        for k, lo, hi in zip(ks.tolist(), first.tolist(), list(first[1:]) + [N]):
            mem = order[lo:hi]                                              # ascending n
            v = data[b, :C][:, mem]
            v = np.where(v > FLOOR, v, -np.inf)                             # NaN > FLOOR is False
            arg = np.argmax(v, axis=1)                                      # the first of the largest
            best = v[np.arange(C), arg]
            out[b, :, k] = np.where(best > -np.inf, mem[arg], 0)
    return out


def index_max_values(data, index, count, K, C=None):
    """-> (max_idx, data[b, c, max_idx] where count > 0 (count None: everywhere), +0.0 elsewhere).  The value carries the
    bits of the entry at max_idx; the kernel's contract differs in ONE point, which no fixture here contains and
    the test named for it pins: a winning -0.0 comes back as +0.0."""
    data = np.asarray(data, np.float32)
    mi = index_max(data, index, K, C)
    val = np.take_along_axis(data[:, :mi.shape[1]], mi.astype(np.int64), axis=2)
    if count is not None:
        val = np.where(np.asarray(count)[:, None, :] > 0, val, np.float32(0))
    return mi, val.astype(np.float32)


def index_max_scatter(g, max_idx, count, N, base=None):
    """base (or zeros) [B,C,N] with g[b,c,k] added at max_idx[b,c,k] for the nodes with count > 0; summed in float64 and
    asserted to be a float32 (dyadic gradients: exact in any order, so the atomic order cannot matter)"""
    g, mi = np.asarray(g, np.float64), np.asarray(max_idx, np.int64)
    B, C, K = g.shape
    out = np.zeros((B, C, N), np.float64) if base is None else np.array(base, np.float64)
    has = np.ones((B, K), bool) if count is None else np.asarray(count) > 0
    for b in range(B):
        for c in range(C):
            np.add.at(out[b, c], mi[b, c][has[b]], g[b, c][has[b]])
    return exact(out, "the scattered gradient") + np.float32(0)


# name -> (seed, B, C, Ctot, N, K, below: nodes per cloud whose members are all <= -1000, nan: NaN members, floors (empty, below))
NODEMAX_CASES = {
    "ch1": (1, 2, 3, 3, 64, 8, 3, 4),
    "ch1_ctot": (2, 2, 3, 5, 128, 16, 4, 6),                                # C < Ctot
    "k1": (3, 2, 2, 2, 16, 1, 0, 2),
    "k257": (4, 1, 2, 2, 1024, 257, 5, 9),                                  # K > 256: the table loops of 256 threads
    "k4096": (5, 1, 2, 2, 1028, 4096, 3, 3),
    "k8192": (6, 1, 1, 1, 64, 8192, 3, 0),                                  # the 64 KiB table
    "n1023": (7, 2, 2, 3, 1023, 32, 3, 7),                                  # N % 4 != 0: the scalar kernels
    "n3": (8, 1, 2, 2, 3, 4, 0, 0),
    "n1": (9, 2, 2, 2, 1, 2, 0, 0),
    "n4": (10, 2, 2, 2, 4, 4, 0, 0),
    "n1028": (11, 1, 2, 2, 1028, 32, 4, 5),
    "n1024": (12, 1, 3, 3, 1024, 64, 6, 5),
    "ch2": (13, 256, 4, 4, 16, 4, 1, 1),                                    # B C / 2 >= 512: two rows per workgroup by shape
    "c8": (14, 2, 8, 9, 64, 8, 3, 4),                                       # four and eight rows per workgroup by knob
}


@functools.lru_cache(maxsize=None)
def nodemax_case(name):
    """-> dict(data [B,Ctot,N], index i32 [B,N] (every value in [0, K)), count i32 [B,K], g [B,C,K], src [B,C+2,N], claims).
    `below` nodes per cloud have all their members at -2000 (index 0 is reported; position 0 collects their gradients);
    NaN members are sprinkled over other nodes; node K - 1 is left empty where K > 1.  claims: empty, below (least per
    cloud), zero_hits (least number of (b, c) nodes that report index 0 without owning it), nan"""
    seed, B, C, Ctot, N, K, below, nan = NODEMAX_CASES[name]
    rng = np.random.default_rng(7000 + seed)
    index = rng.integers(0, max(1, K - 1), (B, N)).astype(np.int32)
    data = dyadic(rng, (B, Ctot, N), 4, 8)
    present = [np.unique(index[b]) for b in range(B)]
    for b in range(B):
        for k in present[b][present[b] != index[b, 0]][:below]:
            data[b][:, index[b] == k] = np.float32(-2000)
        for n in rng.integers(0, N, nan):
            if data[b, 0, n] > FLOOR:
                data[b, rng.integers(0, C), n] = np.nan
    count = np.stack([np.bincount(index[b], minlength=K) for b in range(B)]).astype(np.int32)
    mi = index_max(data, index, K, C)
    stray = [(mi[b] == 0) & (index[b, 0] != np.arange(K))[None, :] & (count[b] > 0)[None, :] for b in range(B)]
    claims = dict(empty=int((count == 0).sum(axis=1).min()), below=min(int(s.sum(axis=1).min()) for s in stray),
                  nan=int(np.isnan(data[:, :C]).sum()))
    assert index.min() >= 0 and index.max() < K
    return dict(data=data, index=index, count=count, g=dyadic(rng, (B, C, K), 4, 8), src=dyadic(rng, (B, C + 2, N), 4, 8),
                claims=claims, C=C, K=K)


# ----------------------------------------------------------------------------------------------- the tail
def softplus64(x):
    """torch.nn.Softplus (beta 1, threshold 20) in float64: x itself above the threshold"""
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def softplus_grad64(x):
    """z / (z + 1), z = exp(x); 1 above the threshold"""
    x = np.asarray(x, np.float64)
    z = np.exp(np.minimum(x, 20.0))
    return np.where(x > 20.0, 1.0, z / (z + 1.0))


def rigid(x, R, scale, shift, transpose=False):
    """out[b,i,m] = shift[b,i] + fma(a2, x2, fma(a1, x1, a0 x0)), a = R[b,i,:] * scale[b] ROUNDED to float32 first (the
    transpose: a = R[b,:,i] * scale[b], no shift); everything after that asserted exact"""
    x, R = np.asarray(x, np.float32), np.asarray(R, np.float32).reshape(-1, 3, 3)
    a = (R.transpose(0, 2, 1) if transpose else R) * np.asarray(scale, np.float32).reshape(-1, 1, 1)
    assert a.dtype == np.float32
    a64, x64 = a.astype(np.float64), x.astype(np.float64)
    t = exact(a64[:, :, 0, None] * x64[:, None, 0], "a0 x0")
    t = exact(a64[:, :, 1, None] * x64[:, None, 1] + t, "fma(a1, x1, .)")
    t = exact(a64[:, :, 2, None] * x64[:, None, 2] + t, "fma(a2, x2, .)")
    return t if transpose else exact(np.asarray(shift, np.float64).reshape(-1, 3, 1) + t, "shift + t")


def loss_combine64(d, chamfer, alpha):
    """-> f64 (chamfer + alpha (mean(d[:half]) + mean(d[half:])), alpha mean(d[:half]), alpha mean(d[half:]))"""
    d = np.asarray(d, np.float64).reshape(-1)
    half = d.size // 2
    m0, m1 = alpha * d[:half].mean(), alpha * d[half:].mean()
    return np.asarray([float(chamfer) + (m0 + m1), m0, m1])


def loss_combine_steps(d, chamfer, alpha):
    """the kernel's steps on sums that are exact in float64 (dyadic d: asserted): m = sum / half * alpha in float64 (alpha the
    float32 it is handed), out0 = chamfer + (m0 + m1) in float64, each of the three rounded to float32 once -> f32 [3]"""
    d = np.asarray(d, np.float64).reshape(-1)
    half = d.size // 2
    assert math.fsum(d[:half]) == float(d[:half].sum()) and math.fsum(d[half:]) == float(d[half:].sum())
    a = float(np.float32(alpha))
    m0 = float(d[:half].sum()) / float(half) * a
    m1 = float(d[half:].sum()) / float(half) * a
    return np.asarray([float(np.float32(chamfer)) + (m0 + m1), m0, m1], np.float64).astype(np.float32)


def adam64(p, g, m, v, t, lr, b1, b2, eps, as_kernel=True):
    """one step of torch.optim.Adam's single-tensor update (no weight decay, no amsgrad) in float64; t = the step count
    AFTER the increment -> (p, m, v).  as_kernel: on the float32 values the kernel is handed -- the hyper-parameters,
    1.0f - beta, and the two bias-correction factors, which it takes in float64 and rounds once"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    r = (lambda h: float(np.float32(h))) if as_kernel else float
    lr, b1, b2, eps = (r(h) for h in (lr, b1, b2, eps))
    one_b1, one_b2 = (r(np.float32(1) - np.float32(b1)), r(np.float32(1) - np.float32(b2))) if as_kernel else (1 - b1, 1 - b2)
    m = m + one_b1 * (g - m)
    v = b2 * v + one_b2 * g * g
    step, bc2s = r(lr / (1.0 - b1 ** t)), r(np.sqrt(1.0 - b2 ** t))
    return p - step * (m / (np.sqrt(v) / bc2s + eps)), m, v


def ulps(got, want64, scale=None):
    """|got - want| in units of 2^-24 |want| (a correctly rounded float32 is within 1), or of 2^-24 scale"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    scale = np.abs(want64) if scale is None else np.asarray(scale, np.float64)
    return np.abs(got - want64) / (2.0 ** -24 * np.maximum(scale, np.finfo(np.float32).tiny))


SIGMA_RAW = (-120.0, -30.0, 0.0, float(np.nextafter(np.float32(20), np.float32(0))), 20.0,
             float(np.nextafter(np.float32(20), np.float32(21))), 25.0, 89.0)


# ----------------------------------------------------------------------------------------------- floors of the claims
# knn_case: (empty cells, longest list, positions whose activation is exactly 0, clamped entries), at most what the seeds give
KNN_FLOORS = {
    "p4": (0, 1, 0, 0), "handover": (1, 37, 4, 0), "handover_odd": (1, 37, 4, 0), "one_list": (4, 128, 0, 0),
    "n513": (40, 5, 0, 2), "n1489": (120, 6, 16, 2), "cout1": (8, 2, 0, 4), "cout9": (0, 38, 24, 4),
    "cout7_p1028": (0, 38, 4, 2), "cout8_p1024": (0, 38, 6, 2), "k1": (0, 8, 0, 4), "p4100": (0, 70, 8, 2),
    "p8196": (0, 135, 40, 2), "p16384": (0, 18, 38, 2), "p16384_odd": (0, 270, 86, 4),
    "chunk2048": (0, 2, 0, 0), "chunk4096": (0, 2, 0, 0), "chunk8320": (0, 2, 0, 0),
}


def knn_claims_hold(name, claims):
    empty, longest, zero_act, clamped = KNN_FLOORS[name]
    lengths = KNN_CASES[name][6]
    return (claims["empty"] >= empty and claims["longest"] >= longest and claims["zero_act"] >= zero_act
            and claims["clamped"] >= clamped and claims["neg_act"] > 0
            and (lengths is None or set(lengths) <= claims["lengths"]))


def nodemax_claims_hold(name, claims):
    _, _, _, _, _, K, below, nan = NODEMAX_CASES[name]
    return claims["empty"] >= (1 if K > 1 else 0) and claims["below"] >= below and claims["nan"] >= nan // 2
