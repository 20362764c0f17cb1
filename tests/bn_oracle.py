"""Plain float64 references of the BatchNorm family (csrc/shared_mlp.hip: bn_finalize, bn_apply, bn_bwd_reduce,
bn_bwd_pool_reduce, bn_bwd_finalize, bn_bwd_finalize_rows; csrc/head.hip: group_dy_sum), numpy and torch on the host,
no GPU.  test_bn_oracle_cpu.py holds them to torch.nn.functional.batch_norm under double autograd; test_bn_kernels_gpu.py
holds the kernels to them.

Conventions: tensors are [nb, C, P] (cloud, channel, position), per-channel vectors [C].  Whatever the kernels read as
fp32 (y, dZ, the forward coefficients, mean, invstd, partial sums) is taken as EXACT and widened to float64; nothing is
rounded on the way except where a kernel's DECISION depends on an fp32 rounding (relu_gate).  Every sum comes with the
sum of the MAGNITUDES of its terms, which is what an error bound counted in roundings multiplies.

The input builders of the GPU tests live here as well (build_case and the *_CASES lists), so that the CPU test can hold
them to the conditions the GPU tests rely on (an empty gate band, fewer than 1 % of the elements moved)."""
import math
import types

import numpy as np
import torch

U = 2.0 ** -24                    # unit roundoff of fp32: one rounding is at most U relative
BAND = 1e-4                       # the gate band of the GPU tests (move_off_the_gate)


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def f64(x):
    return np.asarray(x, dtype=np.float64)


def ulp32(x):
    """spacing of fp32 at the fp32 neighbour of x (float64 array)"""
    return np.spacing(np.abs(f64(x)).astype(np.float32)).astype(np.float64)


def ulps(got32, want64):
    """|got - want| in units of fp32's spacing at `want`; -> float64 array (inf where `got` is not finite)"""
    got, want = f64(got32), f64(want64)
    d = np.abs(got - want) / ulp32(want)
    return np.where(np.isfinite(got), d, np.inf)


def _fsum_last(a):
    """exact (correctly rounded) sum over the last axis"""
    a = f64(a)
    flat = a.reshape(-1, a.shape[-1])
    return np.array([math.fsum(r) for r in flat], dtype=np.float64).reshape(a.shape[:-1])


# ------------------------------------------------------------------------------------------------ forward
def finalize_f64(stats32, count, gamma, beta, eps, momentum, rm, rv):
    """stats32 [2, C, tiles]: fp32 partial sums (row 0) and sums of squares (row 1), summed exactly.
    mean = s/n, var = max(q/n - mean^2, 0), invstd = 1/sqrt(var + eps), coef = (gamma*invstd, beta - mean*gamma*invstd,
    mean, invstd); running statistics (1-m)*r + m*(mean | unbiased var), unbiased = var*n/(n-1) for n > 1, else var.
    eps and momentum are the fp32 values the C entry receives.  gamma None: 1, beta None: 0, rm/rv None: not returned."""
    st = f64(stats32)
    C = st.shape[1]
    n = float(count)
    s, q = _fsum_last(st[0]), _fsum_last(st[1])
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    g = np.ones(C) if gamma is None else f64(gamma)
    b = np.zeros(C) if beta is None else f64(beta)
    scale = g * invstd
    out = types.SimpleNamespace(mean=mean, var=var, invstd=invstd, scale=scale, shift=b - mean * scale,
                                shift_mag=np.abs(b) + np.abs(mean * scale), running_mean=None, running_var=None)
    out.coef = np.stack([out.scale, out.shift, mean, invstd])
    if rm is not None:
        m = float(np.float32(momentum))
        unbiased = var * n / (n - 1.0) if n > 1 else var
        out.running_mean = (1.0 - m) * f64(rm) + m * mean
        out.running_var = (1.0 - m) * f64(rv) + m * unbiased
    return out


def _bc(v):
    return f64(v)[None, :, None]


def relu_gate(y32, sc32, sh32):
    """The gate as the kernels decide it: float32(fma(y, sc, sh)) > 0.  y*sc is exact in float64 (two 24-bit
    significands), so (y*sc + sh) rounded once to fp32 is the fma up to a double rounding that only matters inside the
    band move_off_the_gate empties."""
    t = f64(y32) * _bc(sc32) + _bc(sh32)
    return t.astype(np.float32) > 0


def gate_band(y, sc, sh, band):
    """elements whose fp64 y*sc+sh lies within band*(|y*sc| + |sh|) of zero without being exactly zero"""
    ys, h = f64(y) * _bc(sc), _bc(sh)
    t = ys + h
    return (np.abs(t) <= band * (np.abs(ys) + np.abs(h))) & (t != 0)


def move_off_the_gate(y, sc, sh, band):
    """-> (y', number of elements changed): every element of the band is rewritten so that y'*sc+sh sits at four times
    the band's width on the side it was on; exact zeros (the activation is EXACTLY 0: the gate is closed whatever the
    rounding) stay.  No element's gate then hinges on one rounding."""
    y0 = f32(y)
    y = y0.copy()
    for _ in range(8):
        near = gate_band(y, sc, sh, band)
        if not near.any():
            break
        s, h = _bc(sc), _bc(sh)
        ys = f64(y) * s
        t = ys + h
        target = np.where(t >= 0, 1.0, -1.0) * 4.0 * band * (np.abs(ys) + np.abs(h))
        with np.errstate(divide="ignore", invalid="ignore"):
            ynew = (target - h) / s                                   # s != 0 inside the band (s == 0: t = h, outside or 0)
        y[near] = ynew.astype(np.float32)[near]
    return y, int((y != y0).sum())


# ------------------------------------------------------------------------------------------------ backward
def finalize_partials_f64(s1c, s2c, count, coef32, mean32, invstd32, mx=None, H1c=None, H2c=None):
    """Per channel, from the channel sums s1c = sum dYhat, s2c = sum dYhat*yhat (float64): dbeta, dgamma and the
    coefficients of dY = a1*dYhat + q1*y + q0 = a1*(dYhat - c1m - yhat*c2m):
        row 0 = a1 = coef[0], row 1 = coef[1], row 2 = q1 = -a1*c2m*is, row 3 = q0 = a1*(c2m*is*mu - c1m).
    mag2/mag3: the magnitudes of the terms rows 2 and 3 are summed from (H1c, H2c: sums of |dYhat|, |dYhat*yhat| per
    channel; without them the magnitudes of the final products).  mx (scalar or [C]): max |dYhat|; then `bound` [C] =
    |a1| (mx + |c1m| + |c2m| sqrt(n)) and `row4` = its maximum per 64 channels, the formula of the kernels."""
    n = float(count)
    coef, mu, is_ = f64(coef32), f64(mean32), f64(invstd32)
    a1 = coef[0]
    C = a1.shape[0]
    c1m, c2m = f64(s1c) / n, f64(s2c) / n
    r = types.SimpleNamespace(dbeta=f64(s1c), dgamma=f64(s2c), c1m=c1m, c2m=c2m, count=n, a1=a1, mu=mu, is_=is_)
    r.coef4 = np.stack([a1, coef[1], -a1 * c2m * is_, a1 * (c2m * is_ * mu - c1m)])
    h1 = np.abs(f64(s1c)) if H1c is None else f64(H1c)
    h2 = np.abs(f64(s2c)) if H2c is None else f64(H2c)
    r.mag2 = np.abs(a1 * is_) * h2 / n
    r.mag3 = np.abs(a1) * (np.abs(is_ * mu) * h2 + h1) / n
    if mx is not None:
        r.bound = np.abs(a1) * (f64(mx) + np.abs(c1m) + np.abs(c2m) * math.sqrt(n))
        r.row4 = np.array([r.bound[i:i + 64].max() for i in range(0, C, 64)])
    return r


def reduce_f64(dz32, y32, coef32, mean32, invstd32, relu, group=0):
    """The sums of BatchNorm(+ReLU) backward.  dYhat = dZ * gate (relu_gate; all open without relu),
    yhat = (y - mean) * invstd.
    per row [nb, C]:   s1 = sum dYhat, s2 = sum dYhat*yhat, mx = max |dYhat|, H1 = sum |dYhat|, H2 = sum |dYhat*yhat|
    per channel [C]:   everything of finalize_partials_f64 (dgamma, dbeta, coef4 rows 0-3, bound, row4)
    group = K > 0:     gsum [2, nb, C, P/K] = sums of dYhat and of y over each run of K positions, gmag their magnitudes
    y32 None (plain):  only s1, H1 and dbeta.
    dyh and yhat are kept for callers that want dY itself (dy_f64)."""
    dz = f64(dz32)
    nb, C, P = dz.shape
    if y32 is None:
        return types.SimpleNamespace(s1=dz.sum(-1), H1=np.abs(dz).sum(-1), dbeta=dz.sum((0, 2)), count=float(nb * P))
    y = f64(y32)
    coef = f64(coef32)
    dyh = dz * relu_gate(y32, coef[0], coef[1]) if relu else dz
    yhat = (y - _bc(mean32)) * _bc(invstd32)
    prod = dyh * yhat
    s1, s2 = dyh.sum(-1), prod.sum(-1)
    H1, H2 = np.abs(dyh).sum(-1), np.abs(prod).sum(-1)
    mx = np.abs(dyh).max(-1)
    r = finalize_partials_f64(s1.sum(0), s2.sum(0), nb * P, coef32, mean32, invstd32, mx=mx.max(0),
                              H1c=H1.sum(0), H2c=H2.sum(0))
    r.s1, r.s2, r.mx, r.H1, r.H2, r.dyh, r.yhat = s1, s2, mx, H1, H2, dyh, yhat
    if group:
        G = P // group
        r.gsum = np.stack([dyh.reshape(nb, C, G, group).sum(-1), y.reshape(nb, C, G, group).sum(-1)])
        r.gmag = np.stack([np.abs(dyh).reshape(nb, C, G, group).sum(-1), np.abs(y).reshape(nb, C, G, group).sum(-1)])
    return r


def dy_f64(r):
    """dY = a1 * (dYhat - c1m - yhat * c2m) from reduce_f64's result: the gradient itself, no coefficient form"""
    return r.a1[None, :, None] * (r.dyh - r.c1m[None, :, None] - r.yhat * r.c2m[None, :, None])


def coef_form(coef4, dyh, y):
    """a1*dYhat + q1*y + q0 in float64 from whatever coefficients are handed in"""
    c = f64(coef4)
    return _bc(c[0]) * f64(dyh) + _bc(c[2]) * f64(y) + _bc(c[3])


def coefficient_rounding_bar(r, y):
    """16 U |a1| (|dYhat| + |c1m| + |c2m| is (|y| + |mu|)) per element: what rounding the four coefficients of
    a1*dYhat + q1*y + q0 to fp32 may cost, and nothing more (r: reduce_f64's result)"""
    a = lambda v: np.abs(f64(v))[None, :, None]
    return 16 * U * a(r.a1) * (np.abs(r.dyh) + a(r.c1m) + a(r.c2m) * a(r.is_) * (np.abs(f64(y)) + a(r.mu)))


def forward_mean_rounding_bar(r):
    """U |mu| is |a1| |yhat| |c1m| per element: what the fp32 rounding of the FORWARD mean costs against a gradient taken
    with the exact batch mean (autograd in double).  mean32 = mean (1 + e), |e| <= U, shifts every yhat by
    d = (mean - mean32) is, |d| <= U |mu| is; the sum of dYhat*yhat then holds d * sum dYhat, so c2m becomes c2m + d c1m
    and dY = a1 (dYhat - c1m - yhat c2m) moves by a1 (yhat d c1m + d c2m).  The second part, and the roundings of invstd and
    of a1 = gamma * invstd (2 U of every term), fit into coefficient_rounding_bar's 16 U, of which the coefficients' own
    roundings use at most 9; the first part has no counterpart there: where c2m cancels to nearly nothing (a dZ that is
    uncorrelated with y) while c1m does not, |mu| is = 90 makes it several times the whole bar."""
    a = lambda v: np.abs(f64(v))[None, :, None]
    return U * a(r.mu) * a(r.is_) * a(r.a1) * np.abs(r.yhat) * a(r.c1m)


def pool_scatter(dpooled, arg, K):
    """dense [nb, C, M*K]: dpooled [nb, C, M] at position m*K + arg[nb, C, m] of every neighbourhood, zero elsewhere"""
    dp = np.asarray(dpooled)
    nb, C, M = dp.shape
    dense = np.zeros((nb, C, M, K), dtype=dp.dtype)
    np.put_along_axis(dense, np.asarray(arg, dtype=np.int64)[..., None], dp[..., None], axis=-1)
    return dense.reshape(nb, C, M * K)


def dy_autograd_f64(y, gamma, beta, eps, relu, dz):
    """(dY, dgamma, dbeta) of z = relu?(batch_norm(y)) for the output gradient dz, torch in double under autograd.
    A single sample per channel is refused by F.batch_norm's size check; there the operator it dispatches to is called
    directly (var = 0, yhat = 0)."""
    yt = torch.tensor(f64(y), dtype=torch.float64, requires_grad=True)
    g = torch.tensor(f64(gamma), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(f64(beta), dtype=torch.float64, requires_grad=True)
    if yt.shape[0] * yt.shape[2] > 1:
        z = torch.nn.functional.batch_norm(yt, None, None, g, b, True, 0.1, float(eps))
    else:
        z = torch.batch_norm(yt, g, b, None, None, True, 0.1, float(eps), False)
    if relu:
        z = torch.relu(z)
    z.backward(torch.tensor(f64(dz), dtype=torch.float64))
    return yt.grad.numpy(), g.grad.numpy(), b.grad.numpy()


# ------------------------------------------------------------------------------------------------ input builders
STDS = (0.01, 1.0, 10.0)
DZ_SCALES = (1e-6, 1.0, 1e4)
EPS = 1e-5


def forward_coefficients(y32, gamma32, beta32, eps=EPS):
    """fp32 (mean, invstd, coef [4, C]) of the batch statistics of y32, formed the way bn_finalize forms them"""
    y = f64(y32)
    mean = y.mean((0, 2))
    var = ((y - mean[None, :, None]) ** 2).mean((0, 2))
    mean32 = f32(mean)
    invstd32 = f32(1.0 / np.sqrt(var + float(np.float32(eps))))
    sc32 = f32(gamma32) * invstd32
    sh32 = f32(beta32) - mean32 * sc32
    return mean32, invstd32, np.stack([sc32, sh32, mean32, invstd32])


def build_case(seed, nb, C, P, special=None):
    """_build_once at the first of seed, seed + 1, ... for which the gate condition of the GPU tests holds: the band is
    empty and fewer than 1 % of the elements were moved (a channel 90 deviations off centre with a small beta has more
    than 1 % of its elements in the band; among a handful of elements one moved element is already too many)."""
    for attempt in range(64):
        case = _build_once(seed + attempt, nb, C, P, special)
        if case.band == 0 and case.moved < 0.01 * case.y.size:
            return case
    raise AssertionError("no seed near %d keeps %dx%dx%d off the gate" % (seed, nb, C, P))


def _build_once(seed, nb, C, P, special=None):
    """One input of the backward kernels: y, dz [nb, C, P], gamma, beta, mean, invstd [C], coef [4, C], all fp32.
    Channel c: std = STDS[(c + seed) % 3]; mean uniform in [-50, 50], pulled in to |mean| <= 90 sample deviations so
    that |mu| * is stays under 100 (the q1*y + q0 form loses |mu| * is ulps; see the conditioning test); gamma of
    alternating sign in 0.5 .. 2; dZ of scale DZ_SCALES[(c + c // 3 + seed) % 3].
    Channel 1 (C >= 2) is the ZERO channel: y == 0 and beta == 0, so shift == 0 and the activation is exactly 0.
    Channel 2 (C >= 4) and every channel from 128 on have gamma == 0 (C = 130: the whole third block of 64).
    special (for C == 1): "zero" or "gamma0" makes channel 0 that channel.
    The statistics are those of the final y: statistics and move_off_the_gate are iterated until the band is empty."""
    rng = np.random.default_rng(seed)
    c = np.arange(C)
    std = np.array(STDS)[(c + seed) % 3]
    noise = std[None, :, None] * rng.standard_normal((nb, C, P))
    noise -= noise.mean((0, 2), keepdims=True)
    spread = 90.0 * np.sqrt(noise.var((0, 2)) + EPS)                  # of the SAMPLE: a handful of positions has its own
    mean = np.clip(rng.uniform(-50, 50, C), -spread, spread)
    gamma =rng.uniform(0.5, 2.0, C) * np.where(c % 2 == 0, 1.0, -1.0)
    beta = rng.uniform(-1.0, 1.0, C)
    scale = np.array(DZ_SCALES)[(c + c // 3 + seed) % 3]
    zero = (c == 1) if C >= 2 else np.full(C, special == "zero")
    gamma0 = ((c == 2) & (C >= 4)) | (c >= 128) if C >= 2 else np.full(C, special == "gamma0")
    gamma[gamma0] = 0.0
    beta[zero] = 0.0
    y = mean[None, :, None] + noise
    y[:, zero, :] = 0.0
    y = f32(y)
    dz = f32(scale[None, :, None] * rng.standard_normal((nb, C, P)))
    gamma32, beta32 = f32(gamma), f32(beta)
    y_first = y.copy()
    for _ in range(6):
        mean32, invstd32, coef32 = forward_coefficients(y, gamma32, beta32)
        y, moved = move_off_the_gate(y, coef32[0], coef32[1], BAND)
        if not moved:
            break
    return types.SimpleNamespace(
        y=y, dz=dz, gamma=gamma32, beta=beta32, mean=mean32, invstd=invstd32, coef=coef32, nb=nb, C=C, P=P,
        moved=int((y != y_first).sum()), band=int(gate_band(y, coef32[0], coef32[1], BAND).sum()),
        zero=zero, gamma0=gamma0)


# (nb, C, P, special).  Every loop tail of bn_bwd_reduce_kernel and bn_bwd_finalize_kernel is reached:
#   P 1, 2, 3 .......... scalar path (P % 4 != 0), fewer positions than lanes
#   P 4, 8 ............. vector path, all but one or two lanes read the clamped address P - 4
#   P 1020 ............. one pass, its last lane clamped;  1024: exactly one pass;  1028: one lane in the second pass
#   P 2052, 4100 ....... UNR = 2 and UNR = 4 start a pass of which one sub-iteration holds data
#   nb 1, 7 | 8 | 9, 17  the eight-rows-per-pass loop of bn_bwd_finalize_kernel: tail only | loop only | loop and tail
#   C 1, 63 | 64 | 65, 130: a partial block | a full one | a full one and a partial one (bound row: 1, 1, 2, 3 entries)
DENSE_CASES = [
    (1, 1, 1, None), (7, 1, 2, "zero"), (8, 63, 3, None), (9, 64, 4, None), (17, 65, 8, None),
    (1, 130, 1020, None), (7, 64, 1024, None), (8, 65, 1028, None), (9, 1, 2052, "gamma0"), (1, 63, 4100, None),
    (17, 130, 4, None), (8, 130, 1028, None), (9, 63, 1020, None), (17, 1, 1024, None), (7, 65, 2052, None),
    (1, 64, 3, None), (9, 130, 2, None), (17, 64, 1, None), (8, 1, 4100, None), (1, 65, 1024, None),
    (7, 5, 4100, None),
]

GROUP_KS = (4, 8, 16, 32, 64, 128, 256)


def group_cases():
    """(nb, C, P, K): every lanes-per-group value K/4 = 1 .. 64; P = K (one neighbourhood), 3K, 1024 + K (a row that ends
    inside the second 1024-position pass) and 2048 + 4K (inside the third)"""
    return [(2, 3, P, K) for K in GROUP_KS for P in (K, 3 * K, 1024 + K, 2048 + 4 * K)]


# (nb, C, M, K): M around the 256 lanes of a workgroup; K = 1 (every arg is 0) to 64
POOL_CASES = [
    (1, 1, 1, 1), (2, 65, 255, 3), (3, 5, 256, 16), (2, 3, 257, 64), (1, 2, 600, 64), (9, 64, 600, 1),
    (2, 130, 1, 64), (8, 1, 256, 3), (2, 7, 257, 1), (3, 4, 255, 16), (1, 3, 600, 3),
]


def case_seed(*shape):
    """the seed of a case, from its shape alone: the CPU test checks the very inputs the GPU tests use"""
    s = 7
    for v in shape:
        s = (s * 1000003 + int(v if not isinstance(v, str) else sum(map(ord, v)))) % (1 << 31)
    return s


def build_pool_case(nb, C, M, K):
    """A pooled case: build_case at P = M*K, arg [nb, C, M] int32 uniform in [0, K) with the first row pinned at 0 and
    the last at K - 1, dpooled [nb, C, M] of the channel's dZ scale, yarg = y at the arg-max."""
    case = build_case(case_seed(nb, C, M, K, "pool"), nb, C, M * K)
    rng = np.random.default_rng(case_seed(nb, C, M, K, "arg"))
    arg = rng.integers(0, K, (nb, C, M)).astype(np.int32)
    arg[0, 0, :] = 0
    arg[-1, -1, :] = K - 1
    case.M, case.K, case.arg = M, K, arg
    case.dpooled = np.ascontiguousarray(case.dz.reshape(nb, C, M, K)[..., 0])
    case.yarg = np.ascontiguousarray(np.take_along_axis(case.y.reshape(nb, C, M, K), arg[..., None].astype(np.int64), -1)[..., 0])
    return case


def all_builders():
    """(name, thunk) of every input the GPU file builds, for the CPU test of the gate condition"""
    out = []
    for nb, C, P, sp in DENSE_CASES:
        out.append(("dense %dx%dx%d" % (nb, C, P), lambda a=(nb, C, P, sp): build_case(case_seed(*a[:3]), *a)))
    for nb, C, P, K in group_cases():
        out.append(("group %dx%dx%d K%d" % (nb, C, P, K), lambda a=(nb, C, P): build_case(case_seed(*a, "group"), *a)))
    for nb, C, M, K in POOL_CASES:
        out.append(("pool %dx%dx%dx%d" % (nb, C, M, K), lambda a=(nb, C, M, K): build_pool_case(*a)))
    for what, shapes in (("apply", APPLY_SHAPES + [(2, 3, 1028)]), ("plain", PLAIN_SHAPES), ("refuse", [(2, 3, 1536)]),
                         ("onehot", [(2, 3, P) for P in ONE_HOT_PS])):
        for shape in shapes:
            out.append(("%s %dx%dx%d" % ((what,) + shape), lambda a=shape, w=what: build_case(case_seed(*a, w), *a)))
    for C in BOUND_CS:
        out.append(("bound C%d" % C, lambda C=C: build_case(case_seed(C, "bound"), 3, C, 260)))
    out.append(("conditioning", lambda: build_case(case_seed("conditioning"), *CONDITIONING_SHAPE)))
    return out


APPLY_SHAPES = [(1, 1, 1), (2, 3, 3), (2, 5, 5), (3, 4, 257), (2, 3, 4), (3, 5, 1028), (1, 2, 2052), (2, 65, 1024)]
PLAIN_SHAPES = [(1, 1, 1), (3, 5, 3), (2, 65, 1028), (9, 2, 4100)]
ONE_HOT_PS = (3, 4, 8, 257, 1020, 1024, 1028, 2052, 4100)
BOUND_CS = (1, 64, 65, 130)
CONDITIONING_SHAPE = (5, 67, 1028)


def cancelling_partials(seed, rows, C):
    """[2, rows, C] fp32 partial sums of magnitude 1e6 that cancel to O(1): every value is a multiple of 1/16 (the spacing
    of fp32 at 1e6), so every float64 sum of them, in whatever order, is EXACT (rows * 2^24 < 2^53).  An fp32 chain
    loses the O(1) result entirely."""
    rng = np.random.default_rng(seed)
    pairs = rows // 2
    big = np.round(rng.uniform(0.5e6, 1.0e6, (2, pairs, C)) * 16) / 16
    small = np.round(rng.uniform(-2, 2, (2, pairs + 1, C)) * 16) / 16
    p = np.concatenate([big, small[:, :pairs] - big] + ([small[:, pairs:]] if rows % 2 else []), axis=1)
    p = p[:, rng.permutation(rows)]                                    # (the odd row out has no partner: O(1) itself)
    assert np.array_equal(f32(p).astype(np.float64), p)
    return f32(p)
