"""Plain references of the grouping and pooling kernels (csrc/group.hip) -- the neighbourhood gather and its scatter-add
backward, the first-index max over K with and without the BatchNorm-apply + ReLU in front of it, and its two backwards -- and
the inputs their tests share.  numpy on the CPU only; independent of the library (usip_amd is not imported here).

The inputs are dyadic, so that every reference is exact and every check is on bit patterns:
  y         multiples of 2^-6 within +-8            (a 2^-6, |a| <= 512)
  scales    out of {0.5, 1, 1.5, -0.75, 0, -2}      (b 2^-2, |b| <= 8)
  shifts    multiples of 2^-4 within +-4            (c 2^-4, |c| <= 64), never -0.0
  y s0 + s1 = (a b + 16 c) 2^-8 with |a b + 16 c| <= 5120 < 2^24: exact in float32, so the kernel's fused multiply-add rounds
  nothing and float64 arithmetic reproduces it (act() asserts it); x + (+0.0) is never -0.0, so no activated value is -0.0.
  gradients of the scatter-add: multiples of 2^-4 within +-8; up to 4096 of them sum to at most 2^19 units of 2^-4: exact in
  float32 in ANY order, so the atomic kernel is held to equality although its order is not fixed.

The pooling rule is numpy's arg-max: the first occurrence of the largest value, a NaN counting as the largest (the first
NaN), -0.0 equal to +0.0; the pooled value carries the bits of the entry at that index.  test_group_oracle_cpu.py pins that
this is torch.max(dim=3)'s rule.

Every builder returns, next to the data, what the fixture exists for, and the tests assert these claims against the floors
below (about two thirds of what the seeds used by the tests give on the CPU; none depends on a kernel's answer)."""
import functools

import numpy as np

SCALES = (-0.75, 0.0, 0.5, 1.0, 1.5, -2.0)        # channel c of a table takes SCALES[c]: distinct, c <= 5


def dyadic(rng, shape, log2_step, bound):
    """float32 multiples of 2^-log2_step within +-bound, asserted exact"""
    n = int(bound) << log2_step
    v = rng.integers(-n, n + 1, shape).astype(np.float64) / float(1 << log2_step)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------- dispatch (group.hip:288-430)
def max_kernel_of(K, aligned=True):
    """-> ("max4", L): group_max4_kernel<L>, lane k // 4; or ("max", L): group_max_kernel<L>, lane k % L"""
    L4 = K // 4
    if K % 4 == 0 and L4 & (L4 - 1) == 0 and L4 <= 64 and aligned:
        return "max4", L4
    L = 1
    while L < K and L < 64:
        L <<= 1
    return "max", L


def ragged_rows(K, extra=0):
    """A row count >= K + extra that leaves, in the kernel an aligned z of this K runs, a last workgroup that is partly
    filled and (max4: four rows per thread group, row j of group g = g + j * RPB) thread groups with one and with two of
    their four rows; odd, so that the other kernel family (RPB >= 4) ends on a partial workgroup too."""
    fam, L = max_kernel_of(K)
    rpb = 256 // L
    per, tail = (4 * rpb, rpb + rpb // 2 + 1) if fam == "max4" else (rpb, rpb // 2 + 1)
    rows = -(-(K + extra) // per) * per + tail
    assert rows % 2 == 1 and 0 < tail < per
    return rows


# ----------------------------------------------------------------------------------------------- gather
def gather(x, idx, sub=None, out=None, coff=0):
    """out[b, coff+c, m, k] = x[b, c, idx[b,m,k]] - (c < nsub ? sub[b,c,m] : 0), one float32 subtraction; `out`
    [B,Ctot,M,K] is written in its channel slice only (a copy is returned)"""
    x, idx = np.asarray(x, np.float32), np.asarray(idx)
    B, C, N = x.shape
    _, M, K = idx.shape
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < N), "an index outside the cloud"
    g = np.take_along_axis(x, np.broadcast_to(idx.reshape(B, 1, M * K).astype(np.int64), (B, C, M * K)), axis=2)
    g = g.reshape(B, C, M, K).copy()
    if sub is not None:
        nsub = sub.shape[1]
        g[:, :nsub] = g[:, :nsub] - np.asarray(sub, np.float32)[:, :, :, None]
    assert g.dtype == np.float32
    out = np.empty((B, C, M, K), np.float32) if out is None else np.array(out, np.float32)
    out[:, coff:coff + C] = g
    return out


def scatter_add(dout, idx, C, N, coff=0):
    """dx[b,c,n] = sum over (m,k) with idx[b,m,k] == n of dout[b, coff+c, m, k], summed in float64 and asserted to be a
    float32 (the sum of dyadic gradients is exact) -> float32 [B,C,N]; a point nobody names is +0.0"""
    dout, idx = np.asarray(dout), np.asarray(idx)
    B, Ctot, M, K = dout.shape
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < N), "an index outside the cloud"
    dx = np.zeros((B, C, N), np.float64)
    for b in range(B):
        flat = idx[b].reshape(-1).astype(np.int64)
        for c in range(C):
            np.add.at(dx[b, c], flat, dout[b, coff + c].reshape(-1).astype(np.float64))
    out = dx.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), dx), "the gradients do not sum exactly in float32"
    return out + np.float32(0)                                  # -0.0 + 0.0 = +0.0: an empty sum and a cancelled one are +0.0


def scatter_claims(idx, N):
    """idx i32 [B,M,K] -> dict(same_instr, quarters, unhit), the least over the clouds of: cells that two lanes or more of
    one 64-lane instruction add into; cells added into from two or more of the four waves' quarters of the positions;
    cells nobody names.  A wave's quarter is ((P + 15) / 16) * 4 positions.  same_instr is the smaller of the two lane
    maps: 64 consecutive positions (the scalar LDS kernel; the atomic kernel's waves the same without the quarters), and
    positions base + 4 lane + j (the vector LDS kernel, j = 0..3)."""
    idx = np.asarray(idx)
    B, P = idx.shape[0], idx.shape[1] * idx.shape[2]
    per = ((P + 15) // 16) * 4
    out = []
    for b in range(B):
        flat = idx[b].reshape(-1)
        quarter = np.arange(P) // max(per, 1)
        local = np.arange(P) - quarter * per
        q_of_cell = [set() for _ in range(N)]
        for n, q in zip(flat.tolist(), quarter.tolist()):
            q_of_cell[n].add(q)
        hit = {}
        for name, instr in (("scalar", local // 64), ("vector", (local // 256) * 4 + local % 4)):
            key = (quarter * (P + 1) + instr) * N + flat        # (quarter, instruction, cell)
            uniq, cnt = np.unique(key, return_counts=True)
            hit[name] = len(np.unique(uniq[cnt >= 2] % N))
        out.append(dict(same_instr=min(hit.values()), quarters=sum(len(s) >= 2 for s in q_of_cell),
                        unhit=sum(len(s) == 0 for s in q_of_cell)))
    return {k: min(o[k] for o in out) for k in out[0]} if out else dict(same_instr=0, quarters=0, unhit=N)


# ----------------------------------------------------------------------------------------------- pooling
def first_max(z):
    """z [..., K] float32 -> (pooled [...], arg i32 [...]): np.argmax along the last axis -- first occurrence, a NaN counts
    as the largest; pooled is the entry AT that index (its bits)"""
    z = np.asarray(z, np.float32)
    arg = np.argmax(z, axis=-1)
    pooled = np.take_along_axis(z, arg[..., None], axis=-1)[..., 0]
    return pooled, arg.astype(np.int32)


def act(y, coef, relu):
    """relu?(fma(y, coef[0][c], coef[1][c])) of y [B,C,...]: in float64, asserted exact in float32 (the lattice), so the
    fused multiply-add is reproduced; relu is fmaxf(v, 0): a NaN becomes 0"""
    y, coef = np.asarray(y, np.float32), np.asarray(coef, np.float32)
    C = y.shape[1]
    shape = (1, C) + (1,) * (y.ndim - 2)
    v = y.astype(np.float64) * coef[0].astype(np.float64).reshape(shape) + coef[1].astype(np.float64).reshape(shape)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v, equal_nan=True), "y * s0 + s1 is not exact in float32"
    assert not (np.signbit(out) & (out == 0)).any(), "an activated -0.0: fmaxf(-0.0, 0) is not pinned here"
    if relu:
        out = np.where(out > 0, out, np.float32(0))
    assert out.dtype == np.float32
    return out


def max_act(y, coef, relu):
    """y [B,C,M,K], coef [>=2,C] -> (pooled, arg, yarg): first_max of act(y); yarg = y at the arg-max"""
    pooled, arg = first_max(act(y, coef, relu))
    yarg = np.take_along_axis(np.asarray(y, np.float32), arg[..., None].astype(np.int64), axis=-1)[..., 0]
    return pooled, arg, yarg


def max_backward(dpooled, arg, K):
    """dz[..., k] = dpooled[...] where k == arg[...], else +0.0"""
    dpooled = np.asarray(dpooled, np.float32)
    dz = np.zeros(dpooled.shape + (K,), np.float32)
    np.put_along_axis(dz, np.asarray(arg, np.int64)[..., None], dpooled[..., None], axis=-1)
    return dz


def max_backward_add(dz, dpooled, arg):
    """a copy of dz with dz[..., arg] + dpooled, ONE float32 addition, at the arg-max and every other element as it was"""
    out = np.array(dz, np.float32)
    a = np.asarray(arg, np.int64)[..., None]
    s = np.take_along_axis(out, a, axis=-1)[..., 0] + np.asarray(dpooled, np.float32)
    assert s.dtype == np.float32
    np.put_along_axis(out, a, s[..., None], axis=-1)
    return out


# ----------------------------------------------------------------------------------------------- rows with ties
def tie_claims(z):
    """z [R,K] without NaN -> dict: tied (rows whose maximum is attained twice or more); of those lanes_mod / lanes_div
    (the tied k sit in two lanes or more under k -> k % L of group_max_kernel / k -> k // 4 of group_max4_kernel),
    halves_mod / halves_div (in both 32-lane halves of a wave); rotating (the distinct first arg-max k); constant rows"""
    R, K = z.shape
    _, Lg = max_kernel_of(K, aligned=False)
    c = dict(tied=0, lanes_mod=0, lanes_div=0, halves_mod=0, halves_div=0)
    for r in range(R):
        t = np.flatnonzero(z[r] == z[r].max())
        if len(t) < 2:
            continue
        c["tied"] += 1
        c["lanes_mod"] += len(np.unique(t % Lg)) > 1
        c["lanes_div"] += len(np.unique(t // 4)) > 1
        c["halves_mod"] += len(np.unique((t % Lg) // 32)) > 1
        c["halves_div"] += len(np.unique((t // 4) // 32)) > 1
    c = {k: int(v) for k, v in c.items()}
    c["rotating"] = len(np.unique(np.argmax(z, axis=1)))
    c["constant"] = int((z == z[:, :1]).all(axis=1).sum())
    return c


@functools.lru_cache(maxsize=None)
def tie_rows(seed, R, K):
    """-> (z f32 [R,K] dyadic, claims): values out of about K / 2 levels, so that the maximum is often attained twice or
    more at random places; row r < K has its FIRST maximum at k = r (the rotating maximum: the equal values in front of it
    are lowered by one step); of the rows past K every third is constant."""
    rng = np.random.default_rng(seed)
    n = max(1, K // 4)
    stride = max(1, 511 // n)
    z = (rng.integers(-n, n + 1, (R, K)) * stride).astype(np.float64)
    for r in range(R):
        if r < K:
            m = z[r].max()
            z[r, r] = m
            z[r, :r][z[r, :r] == m] -= 1
        elif (r - K) % 3 == 0:
            z[r] = z[r, 0]
    z /= 64.0
    out = z.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), z) and np.abs(out).max() <= 8
    return out, tie_claims(out)


SPECIAL_ROWS = 6


def special_rows(K):
    """-> z f32 [6,K]: all -inf; +inf twice (at K // 3 and K - 1) among finite values; -0.0 in front of +0.0 among
    negative values, and +0.0 in front of -0.0; subnormals (multiples of 2^-149, the largest twice); a constant row"""
    rng = np.random.default_rng(1000 + K)
    a, b = K // 3, K - 1
    z = np.empty((SPECIAL_ROWS, K), np.float32)
    z[0] = -np.inf
    z[1] = dyadic(rng, K, 6, 8)
    z[1, [a, b]] = np.inf
    for r, (first, second) in ((2, (-0.0, 0.0)), (3, (0.0, -0.0))):
        z[r] = -np.abs(dyadic(rng, K, 6, 8)) - np.float32(0.5)
        z[r, a], z[r, b] = first, second
        if a == b:
            z[r, a] = first
    tiny = np.float32(2.0 ** -149)
    z[4] = rng.integers(-9, 9, K).astype(np.float32) * tiny
    z[4, [a, b]] = np.float32(9) * tiny
    z[5] = np.float32(-3.25)
    assert (np.abs(z[4]) < np.finfo(np.float32).tiny).all() and z[4].max() > 0
    return z


@functools.lru_cache(maxsize=None)
def pool_case(K, R):
    """The rows ops.group_max is tested on -> (z f32 [R,K], claims): tie_rows, and at the ragged row count (R > 3) the six
    special rows after them.  Seed: 100 + K."""
    if R <= 3:
        return tie_rows(100 + K, R, K)
    z, claims = tie_rows(100 + K, R - SPECIAL_ROWS, K)
    return np.concatenate([z, special_rows(K)]), claims


# ----------------------------------------------------------------------------------------------- the activated pool
@functools.lru_cache(maxsize=None)
def act_case(seed, B, C, M, K):
    """-> (y f32 [B,C,M,K], coef f32 [4,C], claims).  Channel c has scale SCALES[c] and a shift that is a multiple of 2^-4
    within +-4; rows 2 and 3 of coef are NaN (the kernel must read rows 0 and 1 only).  From C = 3 on the table holds a
    negative scale (channel 0: the arg-max of the activated values is the arg-MIN of y), a zero scale (channel 1: every
    activated value is the shift, the first k wins) and a channel whose activated values are all <= 0 (channel 2: 0.5 y - 4);
    C = 1 is the negative scale alone.  y takes about K / 2 levels, so that its largest AND its smallest value are often
    attained twice.  claims: tied (rows whose activated maximum, without ReLU, is attained twice or more), negative, zero,
    nonpos (channels of each kind), moved (rows whose arg-max differs from the arg-max of y)."""
    assert 1 <= C <= len(SCALES)
    rng = np.random.default_rng(seed)
    n = max(1, K // 4)
    y = (rng.integers(-n, n + 1, (B, C, M, K)) * max(1, 511 // n)).astype(np.float64) / 64.0
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y) and np.abs(y32).max() <= 8
    coef = np.full((4, C), np.nan, np.float32)
    coef[0] = SCALES[:C]
    coef[1] = dyadic(rng, C, 4, 4) + np.float32(0)
    if C >= 2:
        coef[1, 1] = np.float32(1.25)
    if C >= 3:
        coef[1, 2] = np.float32(-4)
    a = act(y32, coef, False)
    tied = int(((a == a.max(axis=3, keepdims=True)).sum(axis=3) >= 2).sum())
    nonpos = int((a.reshape(B, C, -1).transpose(1, 0, 2).reshape(C, -1) <= 0).all(axis=1).sum())
    moved = int((np.argmax(a, axis=3) != np.argmax(y32, axis=3)).sum())
    claims = dict(tied=tied, negative=int((coef[0] < 0).sum()), zero=int((coef[0] == 0).sum()), nonpos=nonpos, moved=moved)
    return y32, coef, claims


# ----------------------------------------------------------------------------------------------- the cases and their floors
GROUP_MAX_K = (1, 2, 3, 4, 5, 8, 12, 16, 20, 32, 64, 65, 100, 128, 256, 260, 512)
ACT_K = (4, 8, 16, 32, 64, 128, 256)
ACT_SHAPES = ((1, 1, 1), (2, 3, 1), (2, 3, 7), (1, 5, 33))             # (B, C, M)


def act_seed(B, C, M, K):
    return 7000 + 1000 * B + 100 * C + 10 * M + K


# (seed, B, C, N, M, K, channels in front of the slice, channels behind it, what the indices are)
#   idx "random": drawn from the N points; "one": every position names point N // 2
# -> floors (cells with two lanes of one instruction, cells hit from two quarters, cells nobody names), least over the clouds
GATHER_BWD_CASES = {
    "n1_p1": ((61, 2, 3, 1, 1, 1, 2, 1, "random"), (0, 0, 0)),
    "n40_p3": ((62, 2, 3, 40, 3, 1, 1, 2, "random"), (0, 0, 24)),
    "n40_p4": ((63, 2, 5, 40, 1, 4, 3, 1, "random"), (0, 0, 24)),
    "n40_p20": ((64, 2, 3, 40, 5, 4, 1, 1, "random"), (0, 1, 15)),
    "n40_p1028": ((65, 2, 3, 40, 257, 4, 2, 2, "random"), (26, 26, 0)),
    "n40_p1028_one": ((66, 2, 3, 40, 257, 4, 1, 1, "one"), (1, 1, 39)),
    "n2048_p20": ((67, 1, 3, 2048, 5, 4, 1, 1, "random"), (0, 0, 1350)),
    "n2048_p1028": ((68, 2, 3, 2048, 257, 4, 1, 2, "random"), (7, 95, 820)),
    "n2049_p1": ((69, 2, 3, 2049, 1, 1, 1, 1, "random"), (0, 0, 1365)),
    "n2049_p1028": ((70, 2, 5, 2049, 257, 4, 2, 1, "random"), (8, 92, 820)),
    "n4096_p1028": ((71, 2, 3, 4096, 1028, 1, 1, 1, "random"), (3, 58, 2100)),
    "n4096_p1028_one": ((72, 1, 3, 4096, 257, 4, 1, 1, "one"), (1, 1, 4095)),
}


@functools.lru_cache(maxsize=None)
def gather_bwd_case(name):
    """-> (dout f32 [B,Ctot,M,K] with NaN in every channel outside [coff, coff + C), idx i32 [B,M,K], C, N, coff, want f32
    [B,C,N], claims)"""
    (seed, B, C, N, M, K, pre, post, mode), _ = GATHER_BWD_CASES[name]
    rng = np.random.default_rng(seed)
    idx = (rng.integers(0, N, (B, M, K)) if mode == "random" else np.full((B, M, K), N // 2)).astype(np.int32)
    dout = np.full((B, pre + C + post, M, K), np.nan, np.float32)
    dout[:, pre:pre + C] = dyadic(rng, (B, C, M, K), 4, 8)
    assert M * K <= 4096
    return dout, idx, C, N, pre, scatter_add(dout, idx, C, N, pre), scatter_claims(idx, N)


# (B, C, N, M, K, nsub, channels in front, channels behind): P = M K of 1, 255, 256, 257; N = 1; nsub of 0, 3 and C
GATHER_CASES = {
    "p1_n1": (2, 3, 1, 1, 1, 3, 1, 1),
    "p255": (2, 4, 37, 51, 5, 3, 2, 1),
    "p256": (2, 3, 300, 16, 16, 0, 1, 2),
    "p257": (3, 5, 64, 257, 1, 5, 1, 3),
}


@functools.lru_cache(maxsize=None)
def gather_case(name):
    """-> (x f32 [B,C,N], idx i32 [B,M,K] with its first position at point 0 and its last at point N - 1, sub [B,nsub,M] or
    None, coff, Ctot, want f32 [B,Ctot,M,K]: an output filled with SENTINEL, its channel slice written)"""
    B, C, N, M, K, nsub, pre, post = GATHER_CASES[name]
    rng = np.random.default_rng(sum(GATHER_CASES[name]))
    x = dyadic(rng, (B, C, N), 6, 8)
    idx = rng.integers(0, N, (B, M, K)).astype(np.int32)
    idx[:, 0, 0], idx[:, -1, -1] = 0, N - 1
    sub = dyadic(rng, (B, nsub, M), 6, 8) if nsub else None
    out = np.full((B, pre + C + post, M, K), SENTINEL, np.float32)
    return x, idx, sub, pre, pre + C + post, gather(x, idx, sub, out, pre)


SENTINEL = np.float32(-12345.5)


# K -> floors of tie_claims(pool_case(K, ragged_rows(K, SPECIAL_ROWS))): (tied, lanes_mod, lanes_div, halves_mod, halves_div,
# constant), about two thirds of what seed 100 + K gives.  A tie needs two places: it can cross the lanes of k % L from
# K = 2 and those of k // 4 from K = 5, the 32-lane halves of k % 64 from K = 33 and those of k // 4 from K = 129.  At K = 1
# every row is constant.  `rotating` has no floor: it must be K.
POOL_FLOORS = {
    1: (0, 0, 0, 0, 0, 250), 2: (67, 67, 0, 0, 0, 67), 3: (35, 35, 0, 0, 0, 22), 4: (650, 650, 0, 0, 0, 330),
    5: (20, 20, 13, 0, 0, 9), 8: (350, 350, 290, 0, 0, 150), 12: (16, 16, 15, 0, 0, 5), 16: (180, 180, 170, 0, 0, 74),
    20: (12, 12, 9, 0, 0, 2), 32: (88, 88, 86, 0, 0, 31), 64: (68, 68, 66, 50, 0, 18), 65: (27, 27, 26, 16, 0, 1),
    100: (42, 42, 40, 25, 0, 1), 128: (68, 68, 68, 46, 0, 8), 256: (122, 122, 122, 79, 69, 4),
    260: (115, 114, 114, 77, 68, 1), 512: (230, 230, 228, 146, 174, 1),
}
POOL_CLAIMS = ("tied", "lanes_mod", "lanes_div", "halves_mod", "halves_div", "constant")


def pool_claims_hold(K, claims):
    """the ragged case of this K meets its floors and its first maximum visits every k"""
    return claims["rotating"] == K and all(claims[n] >= f for n, f in zip(POOL_CLAIMS, POOL_FLOORS[K]))


# (B, C, M) -> floors (rows whose activated maximum is attained twice, rows whose arg-max is not that of y), at every K
ACT_FLOORS = {(1, 1, 1): (0, 0), (2, 3, 1): (2, 2), (2, 3, 7): (20, 16), (1, 5, 33): (70, 34)}


def act_claims_hold(shape, claims):
    C = shape[1]
    tied, moved = ACT_FLOORS[tuple(shape)]
    return (claims["tied"] >= tied and claims["moved"] >= moved and claims["negative"] == 1
            and claims["zero"] == int(C >= 2) and claims["nonpos"] == int(C >= 3))


def scatter_claims_hold(name, claims):
    same, quarters, unhit = GATHER_BWD_CASES[name][1]
    return claims["same_instr"] >= same and claims["quarters"] >= quarters and claims["unhit"] >= unhit


# ----------------------------------------------------------------------------------------------- NaN
@functools.lru_cache(maxsize=None)
def nan_rows(K):
    """-> (z f32 [2K,K], claims): row k < K holds one NaN, at k, among dyadic values whose maximum is attained once, away
    from k; row K + k holds two, at k and at (7k + 3) % K (one where the two coincide).  The rule: every row pools to NaN
    and arg is the FIRST NaN's k.  claims: first (the distinct k of the first NaN, K), behind (rows whose finite maximum
    sits at a lower k than the first NaN: a kernel that merely skips NaN answers that k), two (rows with two NaNs)."""
    rng = np.random.default_rng(2000 + K)
    z = dyadic(rng, (2 * K, K), 6, 7)
    other = (7 * np.arange(K) + 3) % K
    for r in range(2 * K):
        z[r, (r + K // 2) % K] = np.float32(7.5)              # K = 16: NaN at 2, maximum at 10
        z[r, r % K] = np.nan
        if r >= K:
            z[r, other[r - K]] = np.nan
    isn = np.isnan(z)
    first = np.argmax(isn, axis=1)
    finite_arg = np.argmax(np.where(isn, -np.inf, z), axis=1)
    claims = dict(first=len(np.unique(first)), behind=int((finite_arg < first).sum()), two=int((isn.sum(axis=1) == 2).sum()))
    return z, claims


def nan_floors(K):
    """(distinct first-NaN k, rows whose finite maximum lies in front of the first NaN, rows with two NaNs)"""
    return K, (2 * K) // 4, K - 2
