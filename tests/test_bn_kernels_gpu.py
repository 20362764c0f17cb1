"""The BatchNorm family (csrc/shared_mlp.hip, csrc/head.hip) on the MI355X at its edges, form by form, against the float64
references of tests/bn_oracle.py (which test_bn_oracle_cpu.py anchors to F.batch_norm under double autograd).  Only the
ops.bn_* wrappers, ops.bn_group_dy_sum and the C entries behind them are called: no GEMM, no hand-built bound is consumed.

  bn_finalize_kernel            test_finalize*: the 1024-stride loop and its 256-stride tail (tiles 1 .. 4101), the var < 0
                                clamp, count == 1, gamma / beta / running_* == NULL, a constant channel
  bn_apply_kernel<VEC>          test_apply*: vector and scalar kernel (P % 4, a misaligned view), the slab loop of
                                usip_bn_apply_f32 (nb*C > 65535) with the channel planted in the value, C > 65535 refused,
                                nb*P == 0, NaN under ReLU
  bn_bwd_reduce_kernel<0, UNR>  test_reduce_dense: per-row partials, dgamma, dbeta, coef4 on bn_oracle.DENSE_CASES (clamped
                                loads, scalar path, every tail), UNR = 1, 2, 4 (knob r5_forms 0, 2, 4) bit for bit;
                                test_reduce_one_hot: a clamped load counted twice or a dropped tail; test_reduce_plain
  bn_bwd_reduce_kernel<1, UNR>  test_reduce_group*: lanes per group 1 .. 64, rows ending inside a pass, refusals
  bn_bwd_pool_reduce_kernel     test_pool_reduce: M around 256, K 1 .. 64, arg pinned, yarg against the gather
  bn_bwd_finalize_kernel        through the dense and pooled tests: nb 1, 7 | 8 | 9, 17 (eight-row loop and tail), C % 64
  bn_bwd_finalize_rows_kernel   test_from_partials: rows 1 .. 1000 (16 groups; 8-, 4-, 1-row loops), C % 64, cancelling sums,
                                two parts, maxima of length 1 and 1500
  group_dy_sum_kernel           test_group_dy_sum
  row 4 of coef4                test_bound_row*: every entry, every producer, in f32x2 mode
  the coefficient form          test_conditioning_of_the_coefficient_form

Bars are counted in roundings (U = 2^-24) against sums of magnitudes, not measured.  An fp32 sum over one row:
(ceil(P/256) + 16) U H, H the oracle's magnitude of the row (H1 for s1, H2 for s2): a lane adds at most ceil(P/256) terms,
six shuffle steps, two LDS adds, and the roundings of yhat and of the product make the 16.  Sums taken in double must be the
float64 sum rounded to fp32, within 1 ulp.  Every bar prints its worst err / bar (run with -s).

The worst over all cases, measured on one MI355X (err / bar): row sums s1 0.10, s2 0.15 (grouped 0.07, 0.11; pooled 0.03,
0.10); dgamma 0.10, dbeta 0.07; coef4 rows 2, 3 0.36, 0.40 (from partials 0.30, 0.37); gsum 0.11, 0.12; group_dy_sum 0.47;
finalize coef[1] 0.59; in ulps: mean 0.49, invstd 0.49, coef[0] 0.94 of 2, running statistics 1.34 of 4, apply 0.50 of 1,
one-hot s2 1.05 of 2, the double sums 0.00 of 1.  One bar was widened after a run, by a derived term and not by a constant:
the conditioning check against autograd (its docstring has the figures and the reason).

Mutations this file was run against on an MI355X, one library each, all of them in bounds (wrong values, no wild access),
and the tests that failed:
  min(p, P - 4) -> min(p, max(P - 8, 0)) in both reduce forms ... reduce_dense, reduce_one_hot, reduce_group, bound_row*
  `in` of a clamped sub-iteration always true (counted twice) ....... reduce_dense and reduce_one_hot at r5_forms 2 and 4
      (at UNR = 1 the flag is never false: that form cannot count a clamped load twice)
  the vector loop stops at the last whole 1024-position pass ........ reduce_dense, reduce_one_hot, reduce_group
  the gate `>= 0` instead of `> 0` ................................... reduce_dense, reduce_group, pool_reduce, one_hot
  bn_bwd_finalize_kernel's tail loop drops its last row ............. reduce_dense, reduce_group, pool_reduce, reduce_plain
  its 64-lane maximum of the bound starts at offset 16 .............. bound_row, pool_reduce
  rows kernel: r1 = min(rows, r0 + per + 1): a row counted twice (dropping the clamp altogether reads past the buffer)
      ............................................................... from_partials, bound_row_from_partials
  rows kernel: fp32 chains instead of double ........................ from_partials (27 of its 44 cases)
  rows kernel: max(t0, t1) for the two parts' maxima ................ from_partials, bound_row_from_partials
  pool kernel ignores arg ........................................... pool_reduce
  GROUP form: gy is not reduced across the group's lanes ............ reduce_group
  bn_apply: slabs of 65535 rows (rowid % C taken in a slab that does not start at a channel 0) .. apply_slabs, apply_refuses
  bn_apply: fmaxf(v, -0.f) in the scalar kernel ..................... apply, apply_misaligned_view
  bn_finalize: the 1024-stride loop drops its fourth load ........... finalize (every tiles > 768)
  bn_finalize: no var clamp | unbiased = var n / (n - 1) always ..... finalize_clamps_a_negative_variance_and_takes_one_sample
  group_dy_sum: channel = i % C ..................................... group_dy_sum"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import bn_oracle as bo
from bn_oracle import U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _lib():
    from usip_amd import _lib as L
    return L.lib()


def _ops():
    from usip_amd import ops
    return ops


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _worst(name, err, bound):
    """asserts err <= bound element-wise (err == 0 where the bound is 0) and prints the worst ratio"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    assert np.isfinite(err).all(), name
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print("ratio %-34s %.3f" % (name, ratio))
    assert not err[zero].any(), "%s: a non-zero error where the bar is exactly zero" % name
    assert ratio <= 1.0, "%s: worst err / bar = %.3f" % (name, ratio)
    return ratio


def _within_ulps(name, got, want64, n):
    d = bo.ulps(host(got) if isinstance(got, torch.Tensor) else got, want64)
    print("ulps  %-34s %.3f of %g" % (name, float(d.max()) if d.size else 0.0, n))
    assert (d <= n).all(), "%s: %.3f ulp > %g" % (name, float(d.max()), n)


def _same_bits(a, b, what):
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: not the same bits" % what


def _lanes(P):
    return math.ceil(P / 256) + 16


class _forms:
    """`with _forms(v):` -- knob r5_forms = v, reset on the way out"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        assert _lib().usip_set_tuning(b"r5_forms", self.v) == 0

    def __exit__(self, *exc):
        _lib().usip_set_tuning(b"r5_forms", 0)
        return False


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = _ops().set_matmul_mode(self.mode)

    def __exit__(self, *exc):
        _ops().set_matmul_mode(self.prev)
        return False


class _Dev:
    """the device copies of a bn_oracle case"""

    def __init__(self, case):
        self.case = case
        for k in ("y", "dz", "gamma", "beta", "mean", "invstd", "coef"):
            setattr(self, k, dev(getattr(case, k)))


def _reduce_raw(dz, y, coef, mean, invstd, relu, group=0, want_bound=1):
    """usip_bn_backward_reduce_f32 with test-owned outputs (NaN-filled: whatever is not written shows) ->
    (rc, partial [2|3, nb, C], dgamma, dbeta, coef4, gsum)"""
    nb, C, P = dz.shape
    nan = float("nan")
    partial = torch.full(((3 if want_bound else 2), nb, C), nan, dtype=torch.float32, device=DEV)
    dgamma = torch.full((C,), nan, dtype=torch.float32, device=DEV)
    dbeta = torch.full((C,), nan, dtype=torch.float32, device=DEV)
    coef4 = torch.full((5 if want_bound else 4, C), nan, dtype=torch.float32, device=DEV)
    gsum = torch.full((2, nb, C, P // group), nan, dtype=torch.float32, device=DEV) if group else None
    rc = _lib().usip_bn_backward_reduce_f32(_p(dz), _p(y), _p(coef), _p(mean), _p(invstd), None, int(bool(relu)),
                                            _p(partial), _p(dgamma), _p(dbeta), _p(coef4), _p(gsum), int(group), nb, C, P,
                                            int(want_bound), _stream())
    torch.cuda.synchronize()
    return rc, partial, dgamma, dbeta, coef4, gsum


def _check_sums(tag, r, partial, dgamma, dbeta, coef4, coef_fwd, lanes):
    """per-row partials, channel sums and coefficient rows 0-3 against reduce_f64's result `r`"""
    part = host(partial).astype(np.float64)
    bar1, bar2 = lanes * U * r.H1, lanes * U * r.H2
    _worst(tag + " s1", np.abs(part[0] - r.s1), bar1)
    _worst(tag + " s2", np.abs(part[1] - r.s2), bar2)
    if part.shape[0] > 2:
        assert np.array_equal(part[2], r.mx), tag + ": max |dYhat| per row is exact"
    # the channel sums are double sums of those fp32 rows, rounded once: the rows' bars add up, and one rounding
    _worst(tag + " dbeta", np.abs(host(dbeta) - r.dbeta), bar1.sum(0) + U * np.abs(r.dbeta))
    _worst(tag + " dgamma", np.abs(host(dgamma) - r.dgamma), bar2.sum(0) + U * np.abs(r.dgamma))
    c4 = host(coef4)
    assert np.array_equal(c4[:2].view(np.int32), host(coef_fwd)[:2].view(np.int32)), tag + ": rows 0, 1 are the forward's"
    _worst(tag + " coef4[2]", np.abs(c4[2] - r.coef4[2]), 8 * U * r.mag2)
    _worst(tag + " coef4[3]", np.abs(c4[3] - r.coef4[3]), 8 * U * r.mag3)


# ================================================================================================ bn_finalize
FINALIZE_TILES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 1793, 4101)
TILE = 8
# (mean, std) of channels 0-3; channel 4 is CONSTANT (3.0: its tile sums 24 and 72 are exact).  |mean| / std <= 100: the
# kernel and the oracle both take var = q/n - mean^2 in double, from sums of the same fp32 partials in another order; the
# orders differ by at most tiles * 2^-53 * (q/n) / var = 4101 * 1.1e-16 * 1e4 = 4.5e-9 relative in var, 0.04 ulp of invstd.
FINALIZE_CHANNELS = ((1.0, 0.01), (-50.0, 1.0), (50.0, 10.0), (0.3, 1.0))


@functools.lru_cache(maxsize=None)
def _finalize_case(tiles, C):
    rng = np.random.default_rng(100 * tiles + C)
    y = np.empty((C, tiles, TILE))
    for c in range(C):
        if c == 4:
            y[c] = 3.0
        else:
            m, s = FINALIZE_CHANNELS[(c + tiles) % 4 if C == 1 else c]
            y[c] = bo.f32(m + s * rng.standard_normal((tiles, TILE)))
    stats = bo.f32(np.stack([y.sum(-1), (y * y).sum(-1)]))
    gamma = bo.f32(rng.uniform(0.5, 2.0, C) * np.where(np.arange(C) % 2 == 0, 1, -1))
    beta = bo.f32(rng.uniform(-1, 1, C))
    mean = stats[0].astype(np.float64).sum(-1) / (tiles * TILE)
    rm = bo.f32(0.3 * mean)                   # on the mean's side: the blend does not cancel, its ulp is its terms' ulp
    rv = bo.f32(rng.uniform(0.5, 2.0, C))
    return stats, gamma, beta, rm, rv


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("tiles", FINALIZE_TILES)
def test_finalize(tiles, C):
    """bn_finalize_kernel against finalize_f64: the 1024-stride loop runs for tiles > 768 (1023, 1024, 1025: with 255, 256,
    257 left for the 256-stride tail; 1793 = 1024 + 769: twice for thread 0, once for thread 1; 4101), the tail alone below.
    mean, invstd, coef[0] within 2 ulp; coef[1] within 4 U (|beta| + |mean*scale|); coef[2], coef[3] the bits of mean and
    invstd; running statistics within 4 ulp; C = 5 holds a constant channel: var exactly 0, invstd = rsqrt(eps)."""
    ops = _ops()
    stats, gamma, beta, rm, rv = _finalize_case(tiles, C)
    eps, mom, n = 1e-5, 0.1, tiles * TILE
    f = bo.finalize_f64(stats, n, gamma, beta, eps, mom, rm, rv)
    d_rm, d_rv = dev(rm), dev(rv)
    mean, invstd, coef = ops.bn_finalize(dev(stats), n, dev(gamma), dev(beta), eps, mom, d_rm, d_rv)
    tag = "finalize t%d C%d" % (tiles, C)
    _within_ulps(tag + " mean", mean, f.mean, 2)
    _within_ulps(tag + " invstd", invstd, f.invstd, 2)
    _within_ulps(tag + " coef[0]", coef[0], f.coef[0], 2)
    _worst(tag + " coef[1]", np.abs(host(coef[1]) - f.coef[1]), 4 * U * f.shift_mag)
    _same_bits(coef[2], mean, "coef[2]")
    _same_bits(coef[3], invstd, "coef[3]")
    _within_ulps(tag + " running_mean", d_rm, f.running_mean, 4)
    _within_ulps(tag + " running_var", d_rv, f.running_var, 4)
    if C == 5:
        assert f.var[4] == 0.0
        assert host(invstd)[4] == np.float32(1.0 / np.sqrt(float(np.float32(eps)))) and host(mean)[4] == 3.0
        assert host(d_rv)[4] == (np.float32(1) - np.float32(mom)) * rv[4], "unbiased var of a constant is 0"
    # running statistics not passed: the same coefficients, and nothing else is written
    mean2, invstd2, coef2 = ops.bn_finalize(dev(stats), n, dev(gamma), dev(beta), eps, mom, None, None)
    _same_bits(mean2, mean, "mean without running stats")
    _same_bits(coef2, coef, "coef without running stats")
    # gamma == NULL is 1, beta == NULL is 0
    g = bo.finalize_f64(stats, n, None, None, eps, mom, None, None)
    mean3, invstd3, coef3 = ops.bn_finalize(dev(stats), n, None, None, eps, mom, None, None)
    _same_bits(coef3[0], invstd3, "gamma None: scale is invstd")
    _same_bits(invstd3, invstd, "invstd without gamma")
    _worst(tag + " coef[1] no affine", np.abs(host(coef3[1]) - g.coef[1]), 4 * U * g.shift_mag)
    gb = bo.finalize_f64(stats, n, gamma, None, eps, mom, None, None)
    coef4 = ops.bn_finalize(dev(stats), n, dev(gamma), None, eps, mom, None, None)[2]
    _same_bits(coef4[0], coef[0], "beta None: the same scale")
    _worst(tag + " coef[1] no beta", np.abs(host(coef4[1]) - gb.coef[1]), 4 * U * gb.shift_mag)


def test_finalize_clamps_a_negative_variance_and_takes_one_sample():
    """partials built by hand so that q/n = 8.75 < mean^2 = 9: `var < 0` clamps to 0, invstd = rsqrt(eps), everything finite.
    count == 1: the unbiased variance is var itself (no division by n - 1 = 0); q == s^2 gives var == 0."""
    ops = _ops()
    eps = 1e-5
    rs = np.float32(1.0 / np.sqrt(float(np.float32(eps))))
    stats = dev(bo.f32([[[6.0, 6.0]], [[17.0, 18.0]]]))
    rm, rv = dev(bo.f32([1.0])), dev(bo.f32([2.0]))
    mean, invstd, coef = ops.bn_finalize(stats, 4, dev(bo.f32([2.0])), dev(bo.f32([0.5])), eps, 0.5, rm, rv)
    assert host(mean)[0] == 3.0 and host(invstd)[0] == rs
    assert np.isfinite(host(coef)).all() and host(coef)[0, 0] == np.float32(2.0) * rs
    assert host(rm)[0] == 2.0 and host(rv)[0] == 1.0, "var clamped to 0: running_var = 0.5 * 2 + 0.5 * 0"
    f = bo.finalize_f64(bo.f32([[[6.0, 6.0]], [[17.0, 18.0]]]), 4, [2.0], [0.5], eps, 0.5, [1.0], [2.0])
    _worst("clamp coef[1]", np.abs(host(coef[1]) - f.coef[1]), 4 * U * f.shift_mag)
    # one sample: s = 3, q = 9 (and q = 10: var = 1, the unbiased value is 1 as well, not inf)
    for q, var in ((9.0, 0.0), (10.0, 1.0)):
        rm, rv = dev(bo.f32([1.0])), dev(bo.f32([2.0]))
        mean, invstd, coef = ops.bn_finalize(dev(bo.f32([[[3.0]], [[q]]])), 1, None, None, eps, 0.5, rm, rv)
        f = bo.finalize_f64(bo.f32([[[3.0]], [[q]]]), 1, None, None, eps, 0.5, [1.0], [2.0])
        assert f.var[0] == var and host(mean)[0] == 3.0
        _within_ulps("count 1 invstd", invstd, f.invstd, 2)
        _within_ulps("count 1 running_var", rv, f.running_var, 4)
        assert host(rv)[0] == np.float32(1.0 + 0.5 * var) and host(rm)[0] == 2.0


# ================================================================================================ bn_apply
def _apply_want(y, coef, relu):
    t = bo.f64(y) * bo.f64(coef[0])[None, :, None] + bo.f64(coef[1])[None, :, None]
    return t, (np.maximum(t, 0.0) if relu else t)


def _check_apply(tag, z, y, coef, relu):
    t, want = _apply_want(y, coef, relu)
    z = host(z)
    _within_ulps(tag, z, want, 1)
    if relu:
        below = t < -bo.ulp32(t)
        assert below.any() or t.size < 1000
        assert not z.view(np.int32)[below].any(), tag + ": exactly +0 where the activation is negative"


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", bo.APPLY_SHAPES, ids=str)
def test_apply(shape, relu):
    """bn_apply_kernel: the vector kernel (P % 4 == 0: one lane, a partial block, two blocks) and the scalar one (P 1, 3, 5,
    257), within 1 ulp of the float64 y*sc+sh (the fma rounds once), clamped at 0 under ReLU with +0, never -0"""
    case = bo.build_case(bo.case_seed(*shape, "apply"), *shape)
    z = _ops().bn_apply(dev(case.y), dev(case.coef), relu)
    _check_apply("apply %s" % (shape,), z, case.y, case.coef, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_apply_misaligned_view_takes_the_scalar_kernel(relu):
    """P % 4 == 0 but the tensor starts one float into its allocation: contiguous, not 16-B aligned -> bn_apply_kernel<false>"""
    shape = (2, 3, 1028)
    case = bo.build_case(bo.case_seed(*shape, "apply"), *shape)
    n = case.y.size
    buf = torch.zeros(n + 5, dtype=torch.float32, device=DEV)
    view = buf[1:1 + n].view(shape)
    view.copy_(dev(case.y))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    z = _ops().bn_apply(view, dev(case.coef), relu)
    _check_apply("apply misaligned", z, case.y, case.coef, relu)
    assert not host(buf)[[0, n + 1, n + 2]].any()


@pytest.mark.parametrize("shape", [(3, 30000, 4), (2, 40000, 3)], ids=str)
def test_apply_slabs_keep_the_channel(shape):
    """usip_bn_apply_f32 with nb*C > 65535 rows: slabs of floor(65535/C)*C rows (60000 of 90000: the vector kernel; 40000 of
    80000: the scalar one).  scale 1, shift 8*c, y a small integer: z = y + 8c EXACTLY, so a row that took another channel's
    coefficients after the fold (rowid % C before the slab offset is added) shows."""
    nb, C, P = shape
    rng = np.random.default_rng(C)
    y = rng.integers(0, 8, shape).astype(np.float32)
    coef = np.zeros((4, C), np.float32)
    coef[0] = 1.0
    coef[1] = 8.0 * np.arange(C)
    for relu in (False, True):
        z = host(_ops().bn_apply(dev(y), dev(coef), relu))
        want = y + coef[1][None, :, None]
        bad = np.argwhere(z != want)
        assert len(bad) == 0, "%d rows wrong, first (b, c, p) = %s: channel %g" % (len(bad), tuple(bad[0]), z[tuple(bad[0])] // 8)


def test_apply_refuses_more_than_65535_channels_and_returns_empty():
    """C = 70000 > 65535: no slab holds a whole cloud -> USIP_EINVAL, nothing written.  nb*P == 0: an empty tensor, no launch"""
    ops = _ops()
    C = 70000
    y = torch.ones((1, C, 1), dtype=torch.float32, device=DEV)
    coef = torch.ones((4, C), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="usip_bn_apply_f32"):
        ops.bn_apply(y, coef, True)
    z = torch.full((1, C, 1), -7.0, dtype=torch.float32, device=DEV)
    rc = _lib().usip_bn_apply_f32(_p(y), _p(coef), _p(z), 1, 1, C, 1, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((z == -7.0).all())
    for shape in ((0, 3, 8), (2, 3, 0)):
        out = ops.bn_apply(torch.empty(shape, dtype=torch.float32, device=DEV), coef[:, :3].contiguous(), True)
        assert tuple(out.shape) == shape and out.numel() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", [8, 5], ids=["vector", "scalar"])
def test_apply_and_reduce_close_the_gate_on_nan(P):
    """Under ReLU a NaN input gives 0 (fmaxf returns the other operand), and the reduce kernel closes its gate on the same
    element (NaN > 0 is false): dbeta is the sum of the other elements' dZ, max |dYhat| does not see it."""
    ops = _ops()
    y = np.arange(2 * 2 * P, dtype=np.float32).reshape(2, 2, P) + 1
    y[1, 0, P - 1] = np.nan
    coef = bo.f32([[1.0, 2.0], [0.5, 0.25], [0.0, 0.0], [1.0, 1.0]])
    z = host(ops.bn_apply(dev(y), dev(coef), True))
    assert z[1, 0, P - 1] == 0 and np.isfinite(z).all() and (np.delete(z.ravel(), P * 2 + P - 1) > 0).all()
    dz = np.ones((2, 2, P), np.float32)
    dz[1, 0, P - 1] = 1000.0
    rc, partial, dgamma, dbeta, coef4, _ = _reduce_raw(dev(dz), dev(y), dev(coef), dev(coef[2]), dev(coef[3]), True)
    assert rc == 0
    part = host(partial)
    assert part[0].tolist() == [[P, P], [P - 1, P]] and part[2].tolist() == [[1, 1], [1, 1]]
    assert host(dbeta).tolist() == [2 * P - 1, 2 * P]


# ================================================================================================ bn_backward_reduce, dense
@functools.lru_cache(maxsize=None)
def _dense(shape):
    nb, C, P, sp = shape
    return _Dev(bo.build_case(bo.case_seed(nb, C, P), nb, C, P, sp))


def _dense_oracle(shape, relu):
    c = _dense(shape).case
    return bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", bo.DENSE_CASES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_reduce_dense(shape, relu):
    """bn_bwd_reduce_kernel<false, UNR> + bn_bwd_finalize_kernel on bn_oracle.DENSE_CASES (which names the tail each shape
    reaches): per-row s1, s2 within (ceil(P/256) + 16) U H, max |dYhat| exact; dgamma, dbeta; coef4 rows 0, 1 the forward's
    bits, rows 2, 3 within 8 U of the magnitudes of their terms; where the bar is 0 (the zero channel under ReLU: its gate is
    closed on an activation of exactly 0; a gamma == 0 channel's rows 2, 3) the result is exactly 0.
    UNR = 2 and 4 (knob r5_forms 2, 4) give the bits of UNR = 1; the wrapper gives the bits of the C entry."""
    d = _dense(shape)
    r = _dense_oracle(shape, relu)
    assert d.case.band == 0
    nb, C, P = shape[:3]
    tag = "dense %dx%dx%d %s" % (nb, C, P, "relu" if relu else "lin")
    rc, partial, dgamma, dbeta, coef4, _ = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu)
    assert rc == 0
    _check_sums(tag, r, partial, dgamma, dbeta, coef4, d.coef, _lanes(P))
    if relu and d.case.zero.any():
        assert not host(partial)[:, :, d.case.zero].any(), "the zero channel's gate is closed: strict > 0"
    for form in (2, 4):
        with _forms(form):
            rc, partial_u, dgamma_u, dbeta_u, coef4_u, _ = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu)
        assert rc == 0
        for a, b, what in ((partial_u, partial, "partial"), (dgamma_u, dgamma, "dgamma"), (dbeta_u, dbeta, "dbeta"),
                           (coef4_u[:4], coef4[:4], "coef4")):
            _same_bits(a, b, "%s r5_forms=%d %s" % (tag, form, what))
        _same_bits(coef4_u[4, :(C + 63) // 64], coef4[4, :(C + 63) // 64], "bound row r5_forms=%d" % form)
    og, ob, oc, ogs = _ops().bn_backward_reduce(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, relu)
    assert ogs is None
    _same_bits(og, dgamma, "wrapper dgamma")
    _same_bits(ob, dbeta, "wrapper dbeta")
    _same_bits(oc[:4], coef4[:4], "wrapper coef4")


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_reduce_dense_misaligned_view_takes_the_scalar_path(relu):
    """P % 4 == 0 but dZ starts one float into its allocation: the kernel's `vec` test fails, the scalar loop runs"""
    shape = (2, 3, 1028, None)
    d = _dense(shape)
    r = _dense_oracle(shape, relu)
    n = d.dz.numel()
    buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    view = buf[1:1 + n].view(d.dz.shape)
    view.copy_(d.dz)
    assert view.data_ptr() % 16 == 4
    for dz, y in ((view, d.y), (d.dz, None)):
        if y is None:
            ybuf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
            y = ybuf[1:1 + n].view(d.y.shape)
            y.copy_(d.y)
        rc, partial, dgamma, dbeta, coef4, _ = _reduce_raw(dz, y, d.coef, d.mean, d.invstd, relu)
        assert rc == 0
        _check_sums("misaligned", r, partial, dgamma, dbeta, coef4, d.coef, _lanes(1028))


@pytest.mark.parametrize("shape", bo.PLAIN_SHAPES, ids=str)
def test_reduce_plain(shape):
    """Y == NULL: (None, sum dZ, None, None), the bias gradient of a layer without normalisation"""
    case = bo.build_case(bo.case_seed(*shape, "plain"), *shape)
    r = bo.reduce_f64(case.dz, None, None, None, None, False)
    out = _ops().bn_backward_reduce(dev(case.dz), None, None, None, None, None, False)
    assert out[0] is None and out[2] is None and out[3] is None
    bar = (_lanes(shape[2]) * U * r.H1).sum(0) + U * np.abs(r.dbeta)
    _worst("plain %s" % (shape,), np.abs(host(out[1]) - r.dbeta), bar)


@pytest.mark.parametrize("form", [0, 2, 4], ids=["unr1", "unr2", "unr4"])
@pytest.mark.parametrize("P", bo.ONE_HOT_PS)
def test_reduce_one_hot(P, form):
    """dZ with ONE non-zero per row, at p* in {0, P-4, P-1, 1023, 1024}: s1 is that value EXACTLY and s2 = d * yhat within
    2 ulp (the roundings of y - mean, of * invstd and of the product).  A clamped load min(p, P - 4) that is counted twice
    doubles the value at P-4 .. P-1; a dropped tail loses it: neither can pass."""
    nb, C = 2, 3
    case = bo.build_case(bo.case_seed(nb, C, P, "onehot"), nb, C, P)
    d = _Dev(case)
    spots = sorted({p for p in (0, P - 4, P - 1, 1023, 1024) if 0 <= p < P})
    rng = np.random.default_rng(P)
    for p in spots:
        dz = np.zeros((nb, C, P), np.float32)
        val = bo.f32(rng.uniform(0.5, 2.0, (nb, C)) * np.array([1e-6, 1.0, 1e4])[None, :])
        dz[:, :, p] = val
        for relu in (False, True):
            r = bo.reduce_f64(dz, case.y, case.coef, case.mean, case.invstd, relu)
            with _forms(form):
                rc, partial, _, dbeta, _, _ = _reduce_raw(dev(dz), d.y, d.coef, d.mean, d.invstd, relu)
            assert rc == 0
            part = host(partial)
            assert np.array_equal(part[0].astype(np.float64), r.s1), "P %d p* %d relu %d: s1 %s want %s" % (
                P, p, relu, part[0].tolist(), r.s1.tolist())
            _within_ulps("one-hot P%d p%d s2" % (P, p), part[1], r.s2, 2)
            assert np.array_equal(part[2].astype(np.float64), r.mx)
            if not relu:
                assert np.array_equal(part[0], val)


# ================================================================================================ GROUP form
@functools.lru_cache(maxsize=None)
def _group(shape):
    nb, C, P, K = shape
    return _Dev(bo.build_case(bo.case_seed(nb, C, P, "group"), nb, C, P))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", bo.group_cases(), ids=lambda s: "K%d-P%d" % (s[3], s[2]))
def test_reduce_group(shape, relu):
    """bn_bwd_reduce_kernel<true, UNR>: K/4 = 1 .. 64 lanes per neighbourhood; P = K, 3K, 1024 + K and 2048 + 4K (the row
    ends inside a 1024-position pass: the lanes beyond it shuffle zeros and write nothing).  gsum[0] = sum_k dYhat and
    gsum[1] = sum_k y within (ceil(K/256) + 16) U of their magnitudes; the row sums, dgamma, dbeta and coef4 are the BITS of
    the dense launch on the same data; UNR = 2, 4 give the bits of UNR = 1."""
    nb, C, P, K = shape
    d = _group(shape)
    c = d.case
    r = bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu, group=K)
    rc, partial, dgamma, dbeta, coef4, gsum = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu, group=K)
    assert rc == 0
    g = host(gsum).astype(np.float64)
    tag = "group K%d P%d" % (K, P)
    _worst(tag + " gsum[0]", np.abs(g[0] - r.gsum[0]), _lanes(K) * U * r.gmag[0])
    _worst(tag + " gsum[1]", np.abs(g[1] - r.gsum[1]), _lanes(K) * U * r.gmag[1])
    rc, partial_d, dgamma_d, dbeta_d, coef4_d, _ = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu)
    assert rc == 0
    for a, b, what in ((partial, partial_d, "partial"), (dgamma, dgamma_d, "dgamma"), (dbeta, dbeta_d, "dbeta"),
                       (coef4[:4], coef4_d[:4], "coef4"), (coef4[4, :1], coef4_d[4, :1], "bound")):
        _same_bits(a, b, tag + " against the dense launch: " + what)
    _check_sums(tag, r, partial, dgamma, dbeta, coef4, d.coef, _lanes(P))
    for form in (2, 4):
        with _forms(form):
            rc, partial_u, _, _, coef4_u, gsum_u = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu, group=K)
        assert rc == 0
        _same_bits(gsum_u, gsum, tag + " r5_forms=%d gsum" % form)
        _same_bits(partial_u, partial, tag + " r5_forms=%d partial" % form)
        _same_bits(coef4_u[:4], coef4[:4], tag + " r5_forms=%d coef4" % form)
    out = _ops().bn_backward_reduce(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, relu, group=K)
    _same_bits(out[3], gsum, tag + " wrapper gsum")
    _same_bits(out[0], dgamma, tag + " wrapper dgamma")


def test_reduce_group_refusals():
    """group 6 (no multiple of 4), 12 (K/4 = 3 is no power of two), 512 (more than 64 lanes), P % group != 0, plain mode and a
    view that is not 16-B aligned all raise, before anything is launched"""
    ops = _ops()
    shape = (2, 3, 1536)
    case = bo.build_case(bo.case_seed(*shape, "refuse"), *shape)
    d = _Dev(case)
    for group in (6, 12, 512, 2):
        assert 1536 % group == 0
        with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_f32"):
            ops.bn_backward_reduce(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, True, group=group)
    with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_f32"):
        ops.bn_backward_reduce(d.dz[:, :, :1028].contiguous(), d.y[:, :, :1028].contiguous(), d.coef, d.mean, d.invstd,
                               d.gamma, True, group=8)                           # 1028 % 8 == 4
    n = d.dz.numel()
    for which in ("dz", "y"):
        buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
        view = buf[1:1 + n].view(shape)
        view.copy_(getattr(d, which))
        args = (view, d.y) if which == "dz" else (d.dz, view)
        with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_f32"):
            ops.bn_backward_reduce(*args, d.coef, d.mean, d.invstd, d.gamma, True, group=8)
    rc, partial, _, _, _, gsum = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, True, group=12)
    assert rc != 0 and bool(torch.isnan(partial).all()) and bool(torch.isnan(gsum).all()), "refused: nothing written"
    torch.cuda.synchronize()


# ================================================================================================ pooled
@functools.lru_cache(maxsize=None)
def _pool(shape):
    case = bo.build_pool_case(*shape)
    d = _Dev(case)
    nb, C, M, K = shape
    d.y4 = d.y.view(nb, C, M, K)
    d.arg, d.dpooled, d.yarg = dev(case.arg), dev(case.dpooled), dev(case.yarg)
    return d


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", bo.POOL_CASES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_pool_reduce(shape, relu):
    """bn_bwd_pool_reduce_kernel (+ bn_bwd_finalize_kernel): M = 1, 255, 256, 257, 600 around the 256 lanes, K = 1, 3, 16, 64,
    arg pinned at 0 in the first row and at K - 1 in the last.  With yarg and with the gather: the same bits.  Against
    reduce_f64 on pool_scatter's dense gradient, (ceil(M/256) + 16) U H per row; count = nb*M*K.  In f32x2 mode the partials
    come as a RedSums whose maxima are exact, and row 4 of coef4 bounds the true gradient."""
    ops = _ops()
    nb, C, M, K = shape
    d = _pool(shape)
    c = d.case
    r = bo.reduce_f64(bo.pool_scatter(c.dpooled, c.arg, K), c.y, c.coef, c.mean, c.invstd, relu)
    tag = "pool %dx%dx%dx%d" % shape
    with _mode("f32"):
        dgamma, dbeta, coef4 = ops.bn_pool_backward_reduce(d.dpooled, d.arg, d.y4, d.coef, d.mean, d.invstd, d.gamma, relu)
        dgamma_y, dbeta_y, coef4_y = ops.bn_pool_backward_reduce(d.dpooled, d.arg, d.y4, d.coef, d.mean, d.invstd, d.gamma,
                                                                 relu, yarg=d.yarg)
        part = ops.bn_pool_backward_partials(d.dpooled, d.arg, d.y4, d.coef, d.mean, d.invstd, relu)
        part_y = ops.bn_pool_backward_partials(d.dpooled, d.arg, d.y4, d.coef, d.mean, d.invstd, relu, yarg=d.yarg)
    assert tuple(coef4.shape) == (4, C) and tuple(part.shape) == (2, nb, C)
    for a, b, what in ((dgamma_y, dgamma, "dgamma"), (dbeta_y, dbeta, "dbeta"), (coef4_y, coef4, "coef4"),
                       (part_y, part, "partials")):
        _same_bits(a, b, tag + " with yarg: " + what)
    _check_sums(tag, r, part, dgamma, dbeta, coef4, d.coef, _lanes(M))
    with _mode("f32x2"):
        red = ops.bn_pool_backward_partials(d.dpooled, d.arg, d.y4, d.coef, d.mean, d.invstd, relu, yarg=d.yarg)
        coef5 = ops.bn_pool_backward_reduce(d.dpooled, d.arg, d.y4, d.coef, d.mean, d.invstd, d.gamma, relu)[2]
    assert isinstance(red, ops.RedSums)
    _same_bits(red.sums, part, tag + " RedSums sums")
    assert np.array_equal(host(red.maxima).reshape(nb, C).astype(np.float64), r.mx)
    _same_bits(coef5[:4], coef4, tag + " f32x2 rows 0-3")
    _check_bound_row(tag, host(coef5)[4], r, r.row4)


# ================================================================================================ from partials
@pytest.mark.parametrize("C", [1, 64, 65, 200])
@pytest.mark.parametrize("rows", [1, 2, 15, 16, 17, 31, 63, 64, 100, 127, 1000])
def test_from_partials(rows, C):
    """bn_bwd_finalize_rows_kernel: 16 row groups of ceil(rows/16) rows (rows < 16: groups past the end are empty -- the
    `r1 = min(rows, ...)` clamp; 17, 31: the last groups are short or empty; 100: 7 rows = 4 + 1 + 1 + 1; 127, 1000: the
    8-row loop; 63, 64: the 4-row loop), C % 64 = 0, 1, 8.  Partials of magnitude 1e6, multiples of 1/16, that cancel to
    O(1): every double sum of them is EXACT in whatever order, so dgamma and dbeta must be that sum rounded to fp32 (1 ulp
    allowed); an fp32 chain is off by 0.06 and more.  Rows 0, 1 the forward's bits, rows 2, 3 within 8 U of their terms.
    A list of two parts gives the bits of one; RedSums give the same rows 0-3 and the bound row, maxima of length 1 and
    1500 with the maximum planted at the last index."""
    ops = _ops()
    p = bo.cancelling_partials(1000 * rows + C, rows, C)
    rng = np.random.default_rng(rows + C)
    coef = bo.f32(np.stack([rng.uniform(0.5, 2, C) * rng.choice([-1, 1], C), rng.uniform(-1, 1, C), rng.uniform(-50, 50, C),
                            rng.uniform(0.1, 100, C)]))
    count = 1000
    s = p.astype(np.float64).sum(1)
    r = bo.finalize_partials_f64(s[0], s[1], count, coef, coef[2], coef[3])
    dp, dcoef = dev(p), dev(coef)
    dgamma, dbeta, coef4 = ops.bn_backward_from_partials(dp, count, dcoef, dcoef[2], dcoef[3])
    tag = "rows %d C %d" % (rows, C)
    assert tuple(coef4.shape) == (4, C)
    _within_ulps(tag + " dbeta", dbeta, r.dbeta, 1)
    _within_ulps(tag + " dgamma", dgamma, r.dgamma, 1)
    assert np.array_equal(host(coef4)[:2].view(np.int32), coef[:2].view(np.int32))
    _worst(tag + " coef4[2]", np.abs(host(coef4)[2] - r.coef4[2]), 8 * U * r.mag2)
    _worst(tag + " coef4[3]", np.abs(host(coef4)[3] - r.coef4[3]), 8 * U * r.mag3)
    if rows > 1:
        cut = rows // 2
        two = ops.bn_backward_from_partials([dp[:, :cut].contiguous(), dp[:, cut:].contiguous()], count, dcoef, dcoef[2],
                                            dcoef[3])
        for a, b in zip(two, (dgamma, dbeta, coef4)):
            _same_bits(a, b, tag + " two parts")
    for n0, n1 in ((1, 0), (1500, 0), (1500, 1), (1, 1500)):
        m0 = rng.uniform(0, 1, n0).astype(np.float32)
        m0[-1] = 7.5
        m1 = rng.uniform(0, 1, n1).astype(np.float32)
        if n1:
            m1[-1] = 2.25
        if n1 == 0:
            parts = ops.RedSums(torch.cat([dp.flatten(), dev(m0)]), C, blocks=rows)
            assert parts.maxima.numel() == n0
        else:
            if rows == 1:
                continue
            cut = rows // 2
            parts = [ops.RedSums(torch.cat([dp[:, :cut].flatten(), dev(m0)]), C, blocks=cut),
                     ops.RedSums(torch.cat([dp[:, cut:].flatten(), dev(m1)]), C, blocks=rows - cut)]
        g5, b5, c5 = ops.bn_backward_from_partials(parts, count, dcoef, dcoef[2], dcoef[3])
        assert tuple(c5.shape) == (5, C)
        _same_bits(g5, dgamma, tag + " RedSums dgamma")
        _same_bits(b5, dbeta, tag + " RedSums dbeta")
        _same_bits(c5[:4], coef4, tag + " RedSums coef4")
        rb = bo.finalize_partials_f64(s[0], s[1], count, coef, coef[2], coef[3], mx=7.5 + (2.25 if n1 else 0.0))
        row4 = host(c5)[4, :(C + 63) // 64]
        assert (np.abs(row4 - rb.row4) <= 1e-5 * rb.row4).all(), (tag, n0, n1, row4, rb.row4)


# ================================================================================================ bn_group_dy_sum
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 8), (1, 5, 103, 64), (3, 65, 7, 16), (4, 64, 1, 256), (1, 130, 1, 4)],
                         ids=str)
def test_group_dy_sum(shape):
    """group_dy_sum_kernel: out = K*q0 + a1*g0 + q1*g1 per (cloud, channel, neighbourhood); totals 1, 30, 515, 1365 (no
    multiple of 256: the last block is partial), 256 (exactly one block) and G = 1 (the channel changes with every element),
    within 4 U of the sum of the magnitudes of the three terms"""
    nb, C, G, K = shape
    rng = np.random.default_rng(nb * 1000 + C + G)
    gsum = bo.f32(rng.standard_normal((2, nb, C, G)) * np.array([1.0, 50.0])[:, None, None, None])
    coef4 = bo.f32(rng.standard_normal((4, C)) * np.array([1.0, 1.0, 1e-2, 1e-1])[:, None])
    out = host(_ops().bn_group_dy_sum(dev(gsum), dev(coef4), K))
    c, g = coef4.astype(np.float64), gsum.astype(np.float64)
    t0, t1, t2 = K * c[3][None, :, None] * np.ones_like(g[0]), c[0][None, :, None] * g[0], c[2][None, :, None] * g[1]
    _worst("group_dy_sum %s" % (shape,), np.abs(out - (t0 + t1 + t2)), 4 * U * (np.abs(t0) + np.abs(t1) + np.abs(t2)))


# ================================================================================================ the bound row
def _check_bound_row(tag, row, r, formula):
    """every one of the ceil(C/64) entries of row 4 is at least the true float64 max |dY| of its own 64 channels and equals
    the formula's value for that block within 1e-5 relative; a block whose channels all have a1 == 0 gives exactly 0"""
    C = r.a1.shape[0]
    nblk = (C + 63) // 64
    row = np.asarray(row, np.float64)[:nblk]
    true = np.abs(bo.dy_f64(r)).max((0, 2))
    true = np.array([true[i:i + 64].max() for i in range(0, C, 64)])
    assert np.isfinite(row).all() and (row >= true).all(), "%s: bound %s under the true max |dY| %s" % (tag, row, true)
    assert (np.abs(row - formula) <= 1e-5 * formula).all(), "%s: bound %s, formula %s" % (tag, row, formula)
    for i in range(nblk):
        if not r.a1[64 * i:64 * i + 64].any():
            assert row[i] == 0.0
    print("bound %-34s true/bound %s" % (tag, np.array2string(true / np.maximum(row, 1e-300), precision=3)))


@functools.lru_cache(maxsize=None)
def _bound_case(C):
    return _Dev(bo.build_case(bo.case_seed(C, "bound"), 3, C, 260))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("C", bo.BOUND_CS)
def test_bound_row(C, relu):
    """Row 4 of coef4 as ops.bn_backward_reduce writes it in f32x2 mode, C = 1, 64, 65, 130 (1, 1, 2, 3 entries; C = 130: the
    third block is channels 128, 129, both gamma == 0 -> exactly 0).  The split-fp16 GEMMs scale their streamed operand by
    it: an entry that is too small overflows fp16 planes silently."""
    ops = _ops()
    d = _bound_case(C)
    c = d.case
    r = bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu)
    with _mode("f32x2"):
        dgamma, dbeta, coef5, _ = ops.bn_backward_reduce(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, relu)
    assert tuple(coef5.shape) == (5, C)
    _check_bound_row("reduce C%d" % C, host(coef5)[4], r, r.row4)
    if C == 130:
        assert host(coef5)[4, 2] == 0.0 and r.row4[2] == 0.0


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("C", bo.BOUND_CS)
def test_bound_row_from_partials(C, relu):
    """The row bn_backward_from_partials writes from ONE RedSums (the rows and maxima of a reduce launch) and from TWO (the
    gradient is the sum of two parts: |dYhat| <= max of one + max of the other, over ALL channels): at least the true
    max |dY| of dZ = part a + part b, and the formula's value."""
    ops = _ops()
    d = _bound_case(C)
    c = d.case
    nb, P = c.nb, c.P
    r = bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu)
    rc, partial, _, _, _, _ = _reduce_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu)
    assert rc == 0
    one = ops.RedSums(partial.flatten(), C, blocks=nb)
    assert one.maxima.numel() == nb * C
    c5 = ops.bn_backward_from_partials(one, nb * P, d.coef, d.mean, d.invstd)[2]
    f = bo.finalize_partials_f64(r.dbeta, r.dgamma, nb * P, c.coef, c.mean, c.invstd, mx=r.mx.max())
    _check_bound_row("one RedSums C%d" % C, host(c5)[4], r, f.row4)
    mask = np.random.default_rng(C).random(c.dz.shape) < 0.3
    dza, dzb = np.where(mask, c.dz, np.float32(0)), np.where(mask, np.float32(0), c.dz)
    ra = bo.reduce_f64(dza, c.y, c.coef, c.mean, c.invstd, relu)
    rb = bo.reduce_f64(dzb, c.y, c.coef, c.mean, c.invstd, relu)
    parts = []
    for dzp in (dza, dzb):
        rc, partial, _, _, _, _ = _reduce_raw(dev(dzp), d.y, d.coef, d.mean, d.invstd, relu)
        assert rc == 0
        parts.append(ops.RedSums(partial.flatten(), C, blocks=nb))
    g5, b5, c5 = ops.bn_backward_from_partials(parts, nb * P, d.coef, d.mean, d.invstd)
    f = bo.finalize_partials_f64(r.dbeta, r.dgamma, nb * P, c.coef, c.mean, c.invstd, mx=ra.mx.max() + rb.mx.max())
    _check_bound_row("two RedSums C%d" % C, host(c5)[4], r, f.row4)
    lanes = _lanes(P)
    _worst("two RedSums dbeta", np.abs(host(b5) - r.dbeta), (lanes * U * (ra.H1 + rb.H1)).sum(0) + U * np.abs(r.dbeta))
    _worst("two RedSums dgamma", np.abs(host(g5) - r.dgamma), (lanes * U * (ra.H2 + rb.H2)).sum(0) + U * np.abs(r.dgamma))


# ================================================================================================ conditioning
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_conditioning_of_the_coefficient_form(relu):
    """a1*dYhat + q1*y + q0, reconstructed in float64 from the kernel's fp32 coef4, against dY of F.batch_norm in double
    under autograd.  The form q1*y + q0 cancels: q1*y and q0 are each |mu| * is times larger than their sum a1 c2m yhat, so
    it loses |mu| * is ulps of THAT term (inputs keep |mu| * is <= 100).  That is a property of the form the consumers
    evaluate, stated here and not something this test could change.

    Against the oracle's own dY (the fp32 forward statistics taken as exact, as the kernels take them): 16 U |a1| (|dYhat| +
    |c1m| + |c2m| is (|y| + |mu|)), the rounding of the four coefficients, plus what the bars of the fp32 row sums
    (test_reduce_dense) allow c1m and c2m: |a1| (E1 + |yhat| E2) / n.

    Against autograd, whose statistics are the exact ones: the same 16 U bar plus bn_oracle.forward_mean_rounding_bar.  The
    16 U bar alone was what this test first asserted; it is missed by a factor 2.56 (no ReLU; 0.86 with) on the MI355X -- and
    by 2.50 by the float64 ORACLE on the fp32 statistics, no kernel involved (test_bn_oracle_cpu.py asserts that), in the
    channel with mu * is = -90 whose c2m cancels to 1.3e-10 next to c1m = 2.2e-8: the fp32 rounding of the forward mean
    shifts yhat by up to U |mu| is, which leaks c1m into c2m.  No coefficient rounding is involved and no kernel could do
    better from an fp32 mean, so the term U |mu| is |a1| |yhat| |c1m| is added, derived in forward_mean_rounding_bar; worst
    err / bar with it: 0.35 without ReLU, 0.38 with (against the oracle's own dY: 0.05 and 0.08)."""
    shape = bo.CONDITIONING_SHAPE
    d = _Dev(bo.build_case(bo.case_seed("conditioning"), *shape))
    c = d.case
    nb, C, P = shape
    assert c.band == 0 and (np.abs(bo.f64(c.mean) * bo.f64(c.invstd)) <= 100).all()
    coef4 = host(_ops().bn_backward_reduce(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, relu)[2])[:4]
    r = bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu)
    form = bo.coef_form(coef4, r.dyh, c.y)
    rounding = bo.coefficient_rounding_bar(r, c.y)
    E1, E2 = (_lanes(P) * U * r.H1).sum(0)[None, :, None], (_lanes(P) * U * r.H2).sum(0)[None, :, None]
    sums = np.abs(r.a1)[None, :, None] * (E1 + np.abs(r.yhat) * E2) / (nb * P)
    _worst("conditioning, fp32 statistics", np.abs(form - bo.dy_f64(r)), rounding + sums)
    dy, _, _ = bo.dy_autograd_f64(c.y, c.gamma, c.beta, bo.EPS, relu, c.dz)
    _worst("conditioning, autograd", np.abs(form - dy), rounding + bo.forward_mean_rounding_bar(r))
