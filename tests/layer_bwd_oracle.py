"""Plain references of the fused layer-backward kernels (csrc/layer_bwd_x2.hip, csrc/narrow_bwd.hip) and ONE operand set per
launch that is exact for everything the launch writes.  numpy on the CPU only; independent of the library (usip_amd is not
imported here); the number formats, bounds and prologues come from tests/gemm_oracle.py.

A fused launch forms dY = BatchNorm'(ReLU'(dZ)) and act(X) = relu(fma(x, c0, c1)) on the fly and takes from them
    dX[b][ci][p] = sum_co W[co][ci] dY[b][co][p]            (contraction over co)
    dW[co][ci]   = sum_{b,p} dY[b][co][p] act(X)[b][ci][p]   (contraction over positions; one partial per workgroup)
    RED   s1, s2, max of d = dX [relu on] per workgroup and input channel, GSUM per neighbourhood, WS against a source S
with two fp16 planes per operand and the lo x lo plane product dropped.  layer_fixture hands out operands for which
  * dY, act(X) and W are short dyadic numbers, reproduced exactly by their two planes under the scales the KERNEL derives,
  * per contraction index of EITHER product at most one factor has a low plane,
  * sum |products| stays below 2^24 units for every dX, every dW (over all nb P positions), every per-workgroup sum,
so every output is the fp64 value whatever the order, the tile walk or the wave roles: a form is right iff its outputs EQUAL
the float32 of the fp64 results.  What is restated from the library, and where it was read:
  layer_bwd_blocks, the walk     layer_bwd_x2.hip::layer_bwd_blocks, ::cloud_of (runs of pool_group / 32 tiles with gsum)
  narrow_plan                    narrow_bwd.hip::narrow_plan
  the scales                     layer_bwd_x2.hip: sG = pow2_scale(max coef4[4][0 .. ceil(Cout / 64)), 15), sX from
                                 fabsf(c0) / invstd * sqrtf(nb P) + fabsf(fmaf(mean, c0, c1)), W from the image's trailer
  wsum_finalize                  layer_bwd_x2.hip::wsum_finalize_kernel

The layout.  W has fixed big row PAIRS (16 s, 16 s + 1) = (probe, -almost probe) whose dY rows are small and equal; every other
row pair is (s, -s) with small s.  Every tile of 32 positions holds a dY-low position pair (p, p + 1) in one of those (s, -s) row
pairs -- (v, c) at p, (-c, -v) at p + 1 against equal small act(X): small in dX AND in dW --, an act(X)-low pair (q, q + 1) = (v, c)
in one block of 16 input channels against dY = (1, -1) in one row, and a position where a big W row pair meets a nonzero dY.
dY is steered through y (dY = c2 y + c3 + [on] c0 dZ with c2 = +-1 unit), so the pooled form -- one dZ per run -- reaches the
same targets; dZ is never zero where the mask hides it."""
import math

import numpy as np

from gemm_oracle import (X2H_TOP, _big, assert_exact_sums, backward_bound, exact32, forward_bound, invstd_for_bound,
                         planes_of, pow2_scale, prologue, weight_scale)

BP = 32                                       # positions per tile of layer_bwd_x2_kernel
G_LOG2, X_LOG2, W_LOG2 = 3, 3, 17             # dY = int 2^-3, act(X) = int 2^-3, W = int 2^-17


# ------------------------------------------------------------------------------------------------ the walks
def layer_bwd_blocks(cin, cout, P, nb):
    slots = 256 if (cin == 128 and cout == 128) else 512
    return min(nb * (P // BP), slots)


def layer_walk(cin, cout, P, nb, tpg=1):
    """-> (G, [[(cloud, tile) ...] per workgroup]): workgroup w takes runs w, w + G, ... of tpg consecutive tiles"""
    G = layer_bwd_blocks(cin, cout, P, nb)
    tpc = P // BP
    total = nb * tpc // tpg
    walk = []
    for w in range(G):
        tiles = []
        for r in range(w, total, G):
            tiles += [divmod(r * tpg + i, tpc) for i in range(tpg)]
        walk.append(tiles)
    return G, walk


def narrow_plan(cout, P, nb):
    """-> (seglen, segs); workgroup b * segs + seg takes positions [seg seglen, min(P, (seg + 1) seglen)) of cloud b"""
    slots = 768 if cout == 64 else 512
    per_cloud = max(1, slots // nb)
    tiles = (P + 63) // 64
    tps = max(4, (tiles + per_cloud - 1) // per_cloud)
    seglen = tps * 64
    return seglen, (P + seglen - 1) // seglen


def narrow_walk(cout, P, nb):
    """the same shape as layer_walk, in tiles of 32 positions"""
    seglen, segs = narrow_plan(cout, P, nb)
    return nb * segs, [[(b, t) for t in range(s * seglen // BP, min(P, (s + 1) * seglen) // BP)]
                       for b in range(nb) for s in range(segs)]


# ------------------------------------------------------------------------------------------------ the design
def _design(cin, cout, nb, P, rng, heavy):
    """integer targets: Wi [cout,cin] (units 2^-W_LOG2), Gi = dY [nb,cout,P], Xi = act(X) >= 0 [nb,cin,P], and the roles"""
    tpc = P // BP
    ci = np.arange(cin)
    wb = [(16 * s, 16 * s + 1) for s in range(cout // 16)]
    free = [(k, k + 1) for k in range(0, cout, 2) if k % 16]
    ci_t = cin // 2                                             # the input channel the forward bound comes from
    Wi = np.zeros((cout, cin), np.int64)
    S5 = np.array([1, -1, 2, -2, 0])
    for i, (k0, k1) in enumerate(free):
        Wi[k0] = S5[(ci + i) % 5]
        Wi[k1] = -Wi[k0]
    for s, (k0, k1) in enumerate(wb):
        big = np.array([_big("x2h", int(c) + s) for c in ci])
        Wi[k0], Wi[k1] = big[:, 0], -big[:, 1]
    Wi[:, ci_t] = 0                                             # (its invstd is no power of two: dX stays zero there)
    Gi = (rng.integers(-2, 3, (nb, cout, P)) * (rng.random((nb, cout, P)) < 0.08)).astype(np.int64)
    for k0, k1 in wb:
        Gi[:, k1] = Gi[:, k0]
    Xi = (rng.integers(1, 3, (nb, cin, P)) * (rng.random((nb, cin, P)) < 0.15)).astype(np.int64)
    cx_off, cx_on = 2, 3
    Xi[:, cx_on] = rng.integers(1, 3, (nb, P))
    bound_g = (1 << 14) + 2 + 2 * int(rng.integers(0, 2))     # (never 2^14 itself: its low plane would be empty)
    bound_x = (1 << 14) + 2
    nblk = cin // 16

    def big(j):
        if heavy:                                               # many tiles: the small class only (the dW budget)
            v = 2048 + 2 * (j % 32) + 1
            return v, v - (1 + j % 3)
        return _big("x2h", j)
    for b in range(nb):
        for t in range(tpc):
            T, p0 = b * tpc + t, t * BP
            pl = p0 + 2 * ((3 * T) % 8)
            wl = p0 + (pl - p0 + 2) % 16
            ql = p0 + 16 + 2 * ((5 * T) % 8)
            # dY low: (v, c) at pl, (-c, -v) at pl + 1 in an (s, -s) row pair, equal small act(X)
            k0, k1 = free[T % len(free)]
            v, c = big(T)
            if T == 0:
                v, c = bound_g, bound_g - 64                    # the element on the bound, the next 2^-8 below it
            Gi[b, :, pl:pl + 2] = 0
            Gi[b, k0, pl], Gi[b, k1, pl], Gi[b, k0, pl + 1], Gi[b, k1, pl + 1] = v, c, -c, -v
            Xi[b, :, pl] = Xi[b, :, pl + 1] = np.array([1, 2, 0, 1])[(ci + T) % 4]
            # W low: a big row pair meets a nonzero (small, equal) dY
            w0, w1 = wb[T % len(wb)]
            Gi[b, w0, wl] = Gi[b, w1, wl] = (1 + T % 2) * (-1 if T % 3 == 0 else 1)
            # act(X) low: (v, c) at ql, ql + 1 in one block of 16 channels against dY = (1, -1) in one row
            m0, _ = free[(T + 3) % len(free)]
            Gi[b, :, ql:ql + 2] = 0
            Gi[b, m0, ql], Gi[b, m0, ql + 1] = 1, -1
            Xi[b, :, ql:ql + 2] = 0
            blk = (T % nblk) * 16
            pair = np.array([big(int(c_) + T) for c_ in range(blk, blk + 16)])
            Xi[b, blk:blk + 16, ql], Xi[b, blk:blk + 16, ql + 1] = pair[:, 0], pair[:, 1]
            if T == 0:
                Xi[b, ci_t, ql], Xi[b, ci_t, ql + 1] = bound_x, bound_x - 64
    Xi[:, cx_off] = 0
    # (the always-on channel: equal at a dY-low pair's two positions, small at an act(X)-low pair)
    Xi[:, cx_on] = np.where(Xi[:, cx_on] == 0, 1, Xi[:, cx_on])
    return Wi, Gi, Xi, dict(wb=wb, free=free, ci_t=ci_t, cx_off=cx_off, cx_on=cx_on, ky_off=4, ky_on=5, bound_g=bound_g,
                            bound_x=bound_x)


def _y_side(Gi, roles, rng, pooled):
    """raw (dZ | dpooled, arg), Y, coef4 [5,cout] whose prologue gives exactly Gi 2^-G_LOG2"""
    nb, cout, P = Gi.shape
    gu, yu = 2.0 ** -G_LOG2, 0.25
    co = np.arange(cout)
    c0 = (2.0 ** rng.integers(-1, 2, cout)) * np.where(co % 5 == 2, -1.0, 1.0)
    y0i = rng.integers(-2, 3, cout)
    sig = rng.choice([-1, 1], cout)
    c3i = rng.integers(-1, 2, cout)
    sg = np.sign(c0).astype(np.int64)
    y0i[roles["ky_off"]] = sg[roles["ky_off"]] * (1 << 16)      # never on
    y0i[roles["ky_on"]] = -sg[roles["ky_on"]] * (1 << 16)       # always on
    run_of = np.arange(P)[None, None, :] // max(pooled, 1)
    cz = (1 + (run_of + co[None, :, None]) % 3) * rng.choice([-1, 1], Gi.shape)
    # exact zeros in dZ (they become -0.0): scattered; pooled: never in two neighbouring runs of a channel
    cz = cz * (((run_of + co[None, :, None]) % 11 != 0) if pooled else (rng.random(Gi.shape) < 0.9))
    arg = None
    if pooled:
        runs = P // pooled
        arg = (rng.integers(0, pooled, (nb, cout, 1)) + np.arange(runs)[None, None, :] * (1 + co[None, :, None] % 3)) % pooled
        arg[:, 0::4, 0], arg[:, 1::4, 0], arg[:, 0::4, -1], arg[:, 1::4, -1] = 0, pooled - 1, pooled - 1, 0
        arg[:, 2::4, :], arg[:, 3::4, :] = 0, pooled - 1        # ... and in every run, so that every walk's edges meet both ends
    for k0, k1 in roles["wb"]:                                  # equal rows: one set of coefficients and raw values
        for a in (c0, y0i, sig, c3i, sg):
            a[k1] = a[k0]
        cz[:, k1] = cz[:, k0]
        if pooled:
            arg[:, k1] = arg[:, k0]
    col = lambda a: a[None, :, None]                            # noqa: E731
    if pooled:
        H = np.repeat(arg, pooled, axis=2) == (np.arange(P) % pooled)[None, None, :]
    else:
        H = np.ones(Gi.shape, bool)
    on_of = lambda yi: col(sg) * (yi - col(y0i)) > 0            # noqa: E731
    yB = col(sig) * (Gi - col(c3i))
    yA = col(sig) * (Gi - col(c3i) - cz)
    useA = H & on_of(yA)
    useB = ~useA & (~H | ~on_of(yB))
    flip = ~useA & ~useB                                        # neither is consistent: the other sign of dZ is
    cz = np.where(flip, -cz, cz)
    yi = np.where(useB, yB, col(sig) * (Gi - col(c3i) - cz))
    assert np.all(on_of(yi)[H] == (useA | flip)[H])
    y = yi * yu
    dz = cz * gu / col(c0)                                      # (nonzero also where the mask hides it)
    ties = (yi == col(y0i)) & H & (cz != 0)                     # off, with a dZ that an `>=` would let through
    coef = np.zeros((5, cout))
    coef[0], coef[1], coef[2], coef[3] = c0, -c0 * y0i * yu, sig * gu / yu, c3i * gu
    nent = (cout + 63) // 64
    B = roles["bound_g"] * gu
    coef[4, :] = B * 2.0 ** 20                                  # entries the kernel must not read
    coef[4, :nent] = B / 4
    coef[4, nent - 1] = B
    out = dict(Y=exact32(y, "Y"), coef4=exact32(coef, "coef4"), dZ=None, pool=None, y_ties=int(ties.sum()),
               y_off=bool(not on_of(yi)[:, roles["ky_off"]].any()), y_on=bool(on_of(yi)[:, roles["ky_on"]].all()))
    if pooled:
        dp = np.take_along_axis(dz.reshape(nb, cout, P // pooled, pooled), arg[..., None], axis=3)[..., 0]
        out["pool"] = (exact32(dp, "dpooled"), arg.astype(np.int32), pooled)
    else:
        dz32 = exact32(dz, "dZ")
        out["dZ"] = dz32
    return out


def _x_side(Xi, roles, rng, nb, P, xpro):
    """raw X and xcoef [4,cin] (scale, shift, mean, invstd) with relu(fma(x, c0, c1)) = Xi 2^-X_LOG2 and the kernel's bound on
    bound_x units; xpro False (narrow_bwd without a prologue): X = +-Xi 2^-X_LOG2 as is"""
    _, cin, _ = Xi.shape
    xu = 2.0 ** -X_LOG2
    if not xpro:
        sgn = rng.choice([-1, 1], Xi.shape)
        return dict(X=exact32(Xi * sgn * xu, "X"), xcoef=None, aX=Xi * sgn * xu, pre=None, x_ties=0)
    ci = np.arange(cin)
    c0 = (2.0 ** rng.integers(-1, 2, cin)) * np.where(ci % 5 == 1, -1.0, 1.0)
    c1i = rng.integers(-2, 3, cin)
    mean = rng.integers(-2, 3, cin) * xu
    t = roles["ci_t"]
    c0[t], c1i[t], mean[t] = 1.0, 2, 0.0
    r = int(math.floor(math.log2(math.sqrt(nb * P))))
    j = 14 - X_LOG2 - r
    invstd = np.abs(c0) / 2.0 ** (j - 2)                        # the others: a quarter of the bound (+ the mean term)
    # the tight channel: fl(fl(1 / invstd) sqrtf(nb P)) = (2^14 - k) units and |fma(mean, 1, 2 units)| = (2 + k) units, for the
    # first k at which such an invstd exists
    for k in range(64):
        tight = invstd_for_bound(((1 << 14) - k) * xu, nb, P)
        if tight is not None:
            break
    assert tight is not None, "no invstd puts the derived bound on a short dyadic at this sample count"
    invstd[t], mean[t] = tight, k * xu
    Tp = Xi.astype(np.float64)
    off = Xi == 0
    Tp[off] = -rng.integers(0, 4, int(off.sum()))               # pre-activation 0 (the tie: off) or below
    x = (Tp * xu - (c1i * xu)[None, :, None]) / c0[None, :, None]
    xcoef = exact32(np.stack([c0, c1i * xu, mean, invstd]), "xcoef")
    return dict(X=exact32(x, "X"), xcoef=xcoef, aX=Xi * xu, pre=Tp * xu, x_ties=int((Tp == 0).sum()))


def _neg_zeros(a, every=3):
    z = np.flatnonzero(a.reshape(-1) == 0)
    a.reshape(-1)[z[::every]] = np.float32(-0.0)
    return int(z[::every].size)


def _by_workgroup(per_tile, walk, op="sum"):
    """per_tile [nb, tpc, ...] -> [workgroups, ...]"""
    out = np.zeros((len(walk),) + per_tile.shape[2:])
    for w, tiles in enumerate(walk):
        for b, t in tiles:
            out[w] = out[w] + per_tile[b, t] if op == "sum" else np.maximum(out[w], per_tile[b, t])
    return out


def _tiles(a):
    """[nb, C, P] -> [nb, tpc, C, 32]"""
    nb, C, P = a.shape
    return np.moveaxis(a.reshape(nb, C, P // BP, BP), 2, 1)


def _finish(fx, rec, Wi, roles, ys, xs, nb, P, walk, red, gsum_group, ws_rows, rng, planes, x_rows, ldw, wcol, w_log2=W_LOG2):
    """the fp64 results, the exactness claims, the record"""
    cout, cin = Wi.shape
    gu, xu, wu = 2.0 ** -G_LOG2, 2.0 ** -X_LOG2, 2.0 ** -w_log2
    W = exact32(Wi * wu, "W")
    dY = prologue(3 if ys["pool"] else 2, ys["dZ"], ys["Y"], ys["coef4"], ys["pool"])
    aX = np.asarray(xs["aX"], np.float64)
    if xs["xcoef"] is not None:
        assert np.array_equal(prologue(1, xs["X"], coef=xs["xcoef"]), aX), "the raw X does not give the designed act(X)"
    # ---- exact operands under the kernel's own scales
    if planes:
        bg = backward_bound(ys["coef4"], cout)
        bx = forward_bound(xs["xcoef"], nb, P)
        sG, sX, sW = float(pow2_scale(bg, X2H_TOP)), float(pow2_scale(bx, X2H_TOP)), float(weight_scale(W))
        assert (sG, sX, sW) == (2.0 ** G_LOG2, 2.0 ** X_LOG2, 2.0 ** w_log2), "the kernel's scales are not the designed ones"
        assert float(np.abs(dY).max()) == float(bg) == roles["bound_g"] * gu, "no |dY| on the bound coef4[4]"
        assert float(aX.max()) == float(bx) == roles["bound_x"] * xu, "no act(X) on the forward bound"
        rec["below_bound"] = bool(np.any(np.abs(dY) == (roles["bound_g"] - 64) * gu) and np.any(aX == (roles["bound_x"] - 64) * xu))
        exact32(ys["coef4"][:4].astype(np.float64) * sG, "coef4 sG")
        exact32(xs["xcoef"][:2].astype(np.float64) * sX, "xcoef sX")
        wp = planes_of("x2h", (W.astype(np.float64) * sW).astype(np.float32))
        gp = planes_of("x2h", exact32(dY * sG, "scaled dY"))
        xp = planes_of("x2h", exact32(aX * sX, "scaled act(X)"))
        # dropped lo x lo: per co in dX, per position in dW
        w_lo, g_lo_co = np.any(wp[1] != 0, axis=1), np.any(gp[1] != 0, axis=(0, 2))
        assert not np.any(w_lo & g_lo_co), "dX: a channel with both low planes populated"
        g_lo_p, x_lo_p = np.any(gp[1] != 0, axis=1), np.any(xp[1] != 0, axis=1)
        assert not np.any(g_lo_p & x_lo_p), "dW: a position with both low planes populated"
        # every tile of 32 positions meets a W-low, a dY-low and an act(X)-low product that is kept and nonzero
        w_hit = np.any((gp[0] != 0) & w_lo[None, :, None], axis=1)
        w_hi = np.any(wp[0] != 0, axis=1)
        g_hit = np.any((gp[1] != 0) & w_hi[None, :, None], axis=1) & np.any(xp[0] != 0, axis=1)
        x_hit = x_lo_p & np.any(gp[0] != 0, axis=1)
        edges = np.arange(0, P, BP)
        rec["tiles_without"] = [int((np.add.reduceat(h, edges, axis=1) == 0).sum()) for h in (w_hit, g_hit, x_hit)]
    # ---- the two products
    ulog_dx, ulog_dw = G_LOG2 + w_log2, G_LOG2 + X_LOG2
    tot = np.matmul(np.abs(W.astype(np.float64)).T, np.abs(dY))
    assert float(tot.max()) * 2.0 ** ulog_dx < 2.0 ** 24, "dX: sum |products| reaches 2^24 units"
    dX = np.matmul(W.astype(np.float64).T, dY)
    flat = lambda a: np.moveaxis(a, 1, 0).reshape(a.shape[1], -1)  # noqa: E731
    tot = flat(np.abs(dY)) @ flat(np.abs(aX)).T
    assert float(tot.max()) * 2.0 ** ulog_dw < 2.0 ** 24, "dW: sum |products| over all positions reaches 2^24 units"
    dW = flat(dY) @ flat(aX).T
    fx.update(W=W, dX=exact32(dX, "dX"), dW=exact32(dW, "dW"), dY=dY, aX=aX, walk=walk, blocks=len(walk))
    rec["dx_nonzero"], rec["dw_nonzero"] = int(np.count_nonzero(dX)), int(np.count_nonzero(dW))
    # ---- the producing layer's sums, per workgroup of the walk
    if red:
        xc = xs["xcoef"].astype(np.float64)
        x = xs["X"].astype(np.float64)
        on = xs["pre"] > 0
        d = np.where(on, dX, 0.0)
        xhat = (x - xc[2][None, :, None]) * xc[3][None, :, None]
        jj = int(round(-math.log2(float(xc[3][0] / abs(xc[0][0])))))            # invstd = |c0| 2^-jj, |c0| >= 1/2; x in half units
        ulog_s2 = ulog_dx + X_LOG2 + 1 + max(0, jj + 1)
        dt, st = _tiles(d), _tiles(d * xhat)
        s1, s2 = _by_workgroup(dt.sum(3), walk), _by_workgroup(st.sum(3), walk)
        assert_exact_sums(_by_workgroup(np.abs(dt).sum(3), walk), ulog_dx, (), "s1")
        assert_exact_sums(_by_workgroup(np.abs(st).sum(3), walk), ulog_s2, (), "s2")
        mx = _by_workgroup(np.abs(dt).max(axis=(2, 3)), walk, "max")
        fx["red"] = dict(sums=exact32(np.stack([s1, s2]), "red sums"), maxima=exact32(mx, "red maxima"), d=d)
        tie = xs["pre"] == 0
        rec["x_tie_with_dx"] = int((tie & (dX != 0)).sum())
        rec["x_off_with_dx"] = int((~on & (dX != 0)).sum())
        active = np.array([len(t) > 0 for t in walk])
        rows = np.concatenate([s1, s2, mx[:, None]], axis=1)[active]
        rec["workgroup_rows_differ"] = bool(len(np.unique(rows, axis=0)) == len(rows))
        rec["idle_workgroups"] = int((~active).sum())
        fx["red"]["idle"] = np.flatnonzero(~active)
        if gsum_group:
            g = gsum_group
            dg, xg = d.reshape(nb, cin, P // g, g), x.reshape(nb, cin, P // g, g)
            assert_exact_sums(dg, ulog_dx, 3, "gsum d")
            assert_exact_sums(xg, X_LOG2 + 1, 3, "gsum x")
            fx["red"]["gsum"] = exact32(np.stack([dg.sum(3), xg.sum(3)]), "gsum")
        if ws_rows:
            S = rng.integers(-2, 3, (nb, ws_rows, P)) * 0.5
            S8 = np.zeros((nb, 8, P))
            S8[:, :ws_rows] = S
            xm = x - xc[2][None, :, None]
            St = _tiles(S8)                                                      # [nb, tpc, 8, 32]
            t1 = np.einsum("btcp,btjp->btcj", dt, St)
            t2 = np.einsum("btcp,btjp->btcj", _tiles(xm), St)
            a1 = np.einsum("btcp,btjp->btcj", np.abs(dt), np.abs(St))
            a2 = np.einsum("btcp,btjp->btcj", np.abs(_tiles(xm)), np.abs(St))
            assert_exact_sums(_by_workgroup(a1, walk), ulog_dx + 1, (), "wsum d S")
            assert_exact_sums(_by_workgroup(a2, walk), X_LOG2 + 2, (), "wsum (x - mean) S")
            assert_exact_sums(_by_workgroup(np.abs(St).sum(3), walk), 1, (), "wsum3")
            wsum = np.concatenate([_by_workgroup(t1, walk), _by_workgroup(t2, walk)], axis=2)      # [G][cin][16]
            fx["wsrc"] = exact32(S, "wsrc")
            fx["wsum"], fx["wsum3"] = exact32(wsum, "wsum"), exact32(_by_workgroup(St.sum(3), walk), "wsum3")
            rec["ws_rows_beyond_zero"] = bool(np.all(fx["wsum"][:, :, ws_rows:8] == 0) and
                                              np.all(fx["wsum"][:, :, 8 + ws_rows:] == 0) and np.all(fx["wsum3"][:, ws_rows:] == 0))
            rec["wsum_nonzero"] = int(np.count_nonzero(fx["wsum"]))
    # ---- storage: X as rows of a wider tensor, W as columns of a wider matrix, signed zeros
    X = xs["X"]
    rec["neg_zero"] = [_neg_zeros(X, 5), _neg_zeros(W, 2), _neg_zeros(ys["dZ"], 3) if ys["dZ"] is not None else
                       _neg_zeros(ys["pool"][0], 3)]
    if x_rows and x_rows > cin:
        wide = np.full((nb, x_rows, P), 7.0, np.float32)                        # (the other rows are never read)
        wide[:, :cin] = X
        X = wide
    ldw = ldw or cin
    Wst = np.full((cout, ldw), 3.0, np.float32)
    Wst[:, wcol:wcol + cin] = W
    fx.update(X=X, xcoef=xs["xcoef"], Wst=Wst, wcol=wcol, dZ=ys["dZ"], Y=ys["Y"], coef4=ys["coef4"], pool=ys["pool"])
    rec.update(zeros=bool(np.any(dY == 0) and np.any(aX == 0) and np.any(W == 0)), y_ties=ys["y_ties"], y_off=ys["y_off"],
               y_on=ys["y_on"], x_ties=xs["x_ties"],
               x_off=bool(np.all(aX[:, roles["cx_off"]] == 0)), x_on=bool(np.all(aX[:, roles["cx_on"]] > 0)))
    if ys["pool"]:
        dp, arg, g = ys["pool"]
        rec["arg_first"], rec["arg_last"] = bool(np.any(arg == 0)), bool(np.any(arg == g - 1))
        # at the first and last run of a cloud and of every workgroup's walk some channel sits on either end
        ends = []
        for tiles in walk:
            if tiles:
                ends += [tiles[0], tiles[-1]]
        ends += [(b, 0) for b in range(nb)] + [(b, P // BP - 1) for b in range(nb)]
        runs_at = {(b, t * BP // g) for b, t in ends}
        rec["arg_ends_on_walk_edges"] = sum(1 for b, r in runs_at if np.any(arg[b, :, r] == 0) and np.any(arg[b, :, r] == g - 1))
        rec["walk_edges"] = len(runs_at)
        same = (dp[:, :, 1:] == dp[:, :, :-1]) & (arg[:, :, 1:] == arg[:, :, :-1])
        rec["neighbour_runs_differ"] = bool(not same.any())
    fx["record"] = rec
    return fx


def layer_fixture(cin, cout, nb, P, pooled=0, red=False, gsum=False, ws_rows=0, seed=0, x_rows=0, ldw=0, wcol=0, w_log2=W_LOG2):
    """One exact launch of layer_bwd_x2.hip -> dict(dZ | pool = (dpooled, arg, group), Y, coef4 [5,cout], X [nb, x_rows or
    cin, P], xcoef [4,cin], Wst [cout, ldw] with the operand in columns [wcol, wcol + cin), wsrc [nb, ws_rows, P]; the float32
    of the fp64 results dX, dW, red = dict(sums [2][blocks][cin], maxima [blocks], gsum [2][nb][cin][P / group]), wsum
    [blocks][cin][16], wsum3 [blocks][8]; walk, blocks, record).  w_log2: W = int 2^-w_log2 (any: the kernel scales W by what it
    finds in it)."""
    assert P % 64 == 0 and (not pooled or P % pooled == 0) and (not gsum or (red and pooled and pooled % BP == 0))
    rng = np.random.default_rng(seed * 7919 + cin * 131 + cout * 17 + P + 3 * pooled + nb)
    heavy = nb * (P // BP) > 600
    Wi, Gi, Xi, roles = _design(cin, cout, nb, P, rng, heavy)
    ys = _y_side(Gi, roles, rng, pooled)
    xs = _x_side(Xi, roles, rng, nb, P, True)
    _, walk = layer_walk(cin, cout, P, nb, pooled // BP if gsum else 1)
    rec = dict(shape=(cin, cout, nb, P), pooled=pooled, red=red, gsum=gsum, ws_rows=ws_rows,
               tiles_per_workgroup=sorted({len(t) for t in walk}),
               walk_crosses_clouds=bool(any(len({b for b, _ in t}) > 1 for t in walk)))
    fx = _finish({}, rec, Wi, roles, ys, xs, nb, P, walk, red, pooled if gsum else 0, ws_rows, rng, True, x_rows, ldw, wcol, w_log2)
    assert np.array_equal(fx["dY"], Gi * 2.0 ** -G_LOG2), "the raw operands do not give the designed dY"
    return fx


def narrow_fixture(cout, xpro, red, nb, P, seed=0, x_rows=0, ldw=0, wcol=0):
    """One launch of narrow_bwd.hip (64 inputs): the same operation in exact fp32, so any dyadic operands under the 2^24
    condition do -- the layer design's, without the plane claims; partials by narrow_plan's segments.  xpro False: X is used as
    is (and is signed).  coef4 has four rows."""
    assert P % 64 == 0 and (xpro or not red)
    cin = 64
    rng = np.random.default_rng(seed * 104729 + cout * 31 + P + nb + 2 * xpro + red)
    heavy = nb * (P // BP) > 600
    Wi, Gi, Xi, roles = _design(cin, cout, nb, P, rng, heavy)
    ys = _y_side(Gi, roles, rng, 0)
    xs = _x_side(Xi, roles, rng, nb, P, xpro)
    _, walk = narrow_walk(cout, P, nb)
    seglen, segs = narrow_plan(cout, P, nb)
    rec = dict(shape=(cin, cout, nb, P), xpro=xpro, red=red, seglen=seglen, segs=segs,
               tiles_per_workgroup=sorted({len(t) for t in walk}), x_negative=bool(np.any(xs["aX"] < 0)))
    fx = _finish({}, rec, Wi, roles, ys, xs, nb, P, walk, red, 0, 0, rng, False, x_rows, ldw, wcol)
    fx["coef4"] = np.ascontiguousarray(fx["coef4"][:4])
    return fx


# ------------------------------------------------------------------------------------------------ the finalise kernel
def wsum_finalize_ref(wsum, wsum3, coef4, mean, ws_rows, exact=True):
    """dW[c][j] = a1 S1 + q1 S2 + fma(q1, mu, q0) S3 (j < ws_rows) from wsum [blocks][C][16], wsum3 [blocks][8]; float64, and
    (exact) asserted to be a float32.  The kernel sums and combines in fp64 and rounds ONCE, so for dyadic sums whose
    combination fp64 holds exactly the rounded value is the kernel's too (exact=False: sums of a real launch)."""
    w, w3 = np.asarray(wsum, np.float64), np.asarray(wsum3, np.float64)
    c = np.asarray(coef4, np.float64)
    mu = np.asarray(mean, np.float64)
    t1, t2, t3 = w[:, :, :8].sum(0), w[:, :, 8:].sum(0), w3.sum(0)
    k = exact32(c[2] * mu + c[3], "fma(q1, mu, q0)").astype(np.float64)
    out = c[0][:, None] * t1 + c[2][:, None] * t2 + k[:, None] * t3[None, :]
    return exact32(out[:, :ws_rows], "the finalised weight gradient") if exact else out[:, :ws_rows].astype(np.float32)


def producing_layer(fx, seed=0):
    """The layer that produced X of a WS fixture: hand-built dyadic coef4' [4][cin] = (a1, a0, q1, q0) with (a1, a0) = xcoef[0:2]
    (the mask is the forward's), its batch mean, and its weight gradient dW'[c][j] = sum_{b,p} (a1 d + q1 x + q0) S_j in float64
    -- exact in fp32 for sum |products| < 2^24 units (asserted), so the fp32 weight-gradient kernel must give the same bits as
    the finalised sums."""
    rng = np.random.default_rng(seed)
    xc = fx["xcoef"].astype(np.float64)
    cin = xc.shape[1]
    x = fx["X"][:, :cin].astype(np.float64)
    d = fx["red"]["d"]
    S = fx["wsrc"].astype(np.float64)
    q1 = rng.integers(-1, 2, cin) * 0.125
    q0 = rng.integers(-2, 3, cin) * 0.25
    q1[cin // 2] = 0.0                                          # (the channel whose x reaches the bound: d is zero there anyway)
    dYp = xc[0][None, :, None] * d + q1[None, :, None] * x + q0[None, :, None]
    exact32(dYp, "the producing layer's dY")
    flat = lambda a: np.moveaxis(a, 1, 0).reshape(a.shape[1], -1)  # noqa: E731
    unit = 2.0 ** -60
    tot = flat(np.abs(dYp)) @ flat(np.abs(S)).T
    lsb = np.abs(dYp[dYp != 0]).min() if np.any(dYp != 0) else 1.0
    while unit * 2 <= lsb and np.array_equal(np.round(dYp / (unit * 2)), dYp / (unit * 2)):
        unit *= 2                                               # the coarsest unit every dY' is a multiple of
    assert float(tot.max()) / (unit * 0.5) < 2.0 ** 24, "the producing layer's dW: sum |products| reaches 2^24 units"
    coef4 = exact32(np.stack([xc[0], xc[1], q1, q0]), "coef4'")
    want = exact32(flat(dYp) @ flat(S).T, "the producing layer's dW")
    ref = wsum_finalize_ref(fx["wsum"], fx["wsum3"], coef4, xc[2], S.shape[1])
    assert np.array_equal(ref, want), "the finalised sums are not the producing layer's weight gradient"
    return coef4, exact32(xc[2], "mean"), want


def wsum_synthetic(blocks, C, ws_rows, seed=0):
    """dyadic per-workgroup sums and coefficients for which wsum_finalize_ref is exact; no two workgroups alike, so a slice of
    the finalise kernel's 32-slice / 8-unrolled / tail loop that is skipped or taken twice shows"""
    rng = np.random.default_rng(seed + 31 * blocks + ws_rows)
    wsum = rng.integers(-8, 9, (blocks, C, 16)) * 0.25 + np.arange(blocks)[:, None, None] * 0.25
    wsum3 = rng.integers(1, 9, (blocks, 8)) * 0.5 + np.arange(blocks)[:, None] * 0.5      # (positive: S3 never sums to zero)
    coef4 = np.zeros((4, C))
    coef4[0] = 2.0 ** rng.integers(-1, 2, C) * rng.choice([-1, 1], C)
    coef4[1] = 99.0                                            # (not read)
    coef4[2] = rng.integers(-3, 4, C) * 0.125
    coef4[3] = rng.integers(-3, 4, C) * 0.25
    mean = rng.integers(1, 4, C) * 0.5                         # never zero: fma(q1, mu, q0) differs from q0 wherever q1 != 0
    return exact32(wsum, "wsum"), exact32(wsum3, "wsum3"), exact32(coef4, "coef4"), exact32(mean, "mean")


# ------------------------------------------------------------------------------------------------ the BatchNorm finalisation
def bn_finalize_ref(sums, maxima, count, xcoef):
    """What usip_bn_backward_finalize_max_f32 (shared_mlp.hip::bn_bwd_finalize_rows_kernel) makes of partials [2][rows][C] and
    maxima: the row sums in float64 (exact for a fixture's partials) -> dgamma = f32(sum s2), dbeta = f32(sum s1), and coef4
    [5][C]: rows 0, 1 copied from xcoef; c1m = f32(s1 / n), c2m = f32(s2 / n); rows 2, 3 = -a1 c2m invstd and
    a1 (c2m invstd mean - c1m), one float32 operation after the other as the kernel writes them (with power-of-two a1, invstd and
    mean every product is exact and only the subtraction rounds, once); row 4, one entry per 64 channels =
    max |a1| ((max + |c1m|) + |c2m| f32(sqrt n))."""
    f = np.float32
    s = np.asarray(sums, np.float64).sum(1)
    xc = np.asarray(xcoef, f)
    C = xc.shape[1]
    a1, a0, mu, inv = xc[0], xc[1], xc[2], xc[3]
    c1m, c2m = (s[0] / float(count)).astype(f), (s[1] / float(count)).astype(f)
    q1 = ((-a1) * c2m).astype(f) * inv
    q0 = a1 * ((((c2m * inv).astype(f) * mu).astype(f) - c1m).astype(f))
    mx = f(np.asarray(maxima, f).max())
    bound = np.abs(a1) * (((mx + np.abs(c1m)).astype(f) + (np.abs(c2m) * f(math.sqrt(float(count)))).astype(f)).astype(f))
    coef4 = np.zeros((5, C), f)
    coef4[0], coef4[1], coef4[2], coef4[3] = a1, a0, q1.astype(f), q0.astype(f)
    nent = (C + 63) // 64
    coef4[4, :nent] = [bound[64 * i:64 * i + 64].max() for i in range(nent)]
    return s[1].astype(f), s[0].astype(f), coef4, nent


def true_dy_maxima(fx, coef4):
    """max |a1 d + q1 x + q0| per 64 input channels, float64: what row 4 of bn_finalize_ref's coef4 has to cover"""
    c = np.asarray(coef4, np.float64)
    cin = c.shape[1]
    x = fx["X"][:, :cin].astype(np.float64)
    dy = np.abs(c[0][None, :, None] * fx["red"]["d"] + c[2][None, :, None] * x + c[3][None, :, None])
    return np.array([dy[:, 64 * i:64 * i + 64].max() for i in range((cin + 63) // 64)])
