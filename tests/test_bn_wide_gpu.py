"""The BatchNorm-backward reduction for neighbourhoods wider than 256 samples (csrc/group_wide.hip: bn_bwd_reduce_wide_kernel<NP>
+ bn_bwd_finalize_kernel) against bn_oracle.reduce_f64(group=K), which makes no assumption about K.

One workgroup per (cloud, channel) row; wave w of four walks the neighbourhoods w, w + 4, ...; lane l owns the float4s l + 64 j,
j < NP = ceil(K / 256).  The cases:
  (1, 1, 260, 260)     one neighbourhood, one lane in the second pass, three waves idle
  (2, 3, 896, 448)     two neighbourhoods: two waves idle
  (1, 2, 2240, 448)    five: wave 0 takes two
  (3, 2, 2880, 320)    nine; nb = 3
  (1, 2, 2048, 512)    both passes whole
  (1, 2, 4080, 1020)   four passes, the last lane of the last one idle
  (2, 65, 3072, 1024)  four whole passes; C = 65: two blocks of the finalisation

Bars, counted in roundings of the order the kernel implements (U = 2^-24), against the oracle's sums of magnitudes; nothing
is fitted:
  row sums s1, s2   a lane takes 4 NP ceil(G / 4) elements (G = P / K neighbourhoods, a quarter of them per wave): s2 is one
                    fma per element, s1 one addition per float4 behind the two of (d0 + d1) + (d2 + d3); then six shuffle
                    steps and two LDS additions, and for s2 the roundings of y - mean, of * invstd and of the product: at
                    most 11, counted as 16 as tests/test_bn_kernels_gpu.py does.  Bar (4 NP ceil(G / 4) + 16) U H.
  gsum              two roundings of the float4's sum, NP - 1 additions of the passes, six butterfly steps: (NP + 7) U gmag.
  dgamma, dbeta, coef4 rows 2, 3: test_bn_kernels_gpu._check_sums with the row bar above.
max |dYhat| per row is exact.  Every bar prints its worst err / bar (run with -s).

The worst over all cases, measured on one MI355X (err / bar): gsum[0] 0.036, gsum[1] 0.203; row sums s1 0.006, s2 0.009;
dbeta 0.006, dgamma 0.006; coef4 rows 2, 3 0.019, 0.015.  The finalisation from partial sums gave the same bits everywhere."""
import math

import numpy as np
import pytest
import torch

import bn_oracle as bo
from bn_oracle import U
from test_bn_kernels_gpu import DEV, _check_sums, _Dev, _lib, _ops, _p, _same_bits, _stream, _worst, host

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 260, 260), (2, 3, 896, 448), (1, 2, 2240, 448), (3, 2, 2880, 320), (1, 2, 2048, 512), (1, 2, 4080, 1020),
         (2, 65, 3072, 1024)]
_CACHE = {}


def _case(shape):
    if shape not in _CACHE:
        nb, C, P, K = shape
        _CACHE[shape] = _Dev(bo.build_case(bo.case_seed(nb, C, P, "wide"), nb, C, P))
    return _CACHE[shape]


def _row_lanes(P, K):
    return 4 * math.ceil(K / 256) * math.ceil(P // K / 4) + 16


def _reduce_wide_raw(dz, y, coef, mean, invstd, relu, group, want_bound=1, gsum=True):
    """usip_bn_backward_reduce_wide_f32 with test-owned outputs (NaN-filled: whatever is not written shows) ->
    (rc, partial [2|3, nb, C], dgamma, dbeta, coef4, gsum)"""
    nb, C, P = dz.shape
    nan = float("nan")
    partial = torch.full(((3 if want_bound else 2), nb, C), nan, dtype=torch.float32, device=DEV)
    dgamma = torch.full((C,), nan, dtype=torch.float32, device=DEV)
    dbeta = torch.full((C,), nan, dtype=torch.float32, device=DEV)
    coef4 = torch.full((5 if want_bound else 4, C), nan, dtype=torch.float32, device=DEV)
    gs = torch.full((2, nb, C, max(1, P // max(group, 1))), nan, dtype=torch.float32, device=DEV) if gsum else None
    rc = _lib().usip_bn_backward_reduce_wide_f32(_p(dz), _p(y), _p(coef), _p(mean), _p(invstd), None, int(bool(relu)),
                                                 _p(partial), _p(dgamma), _p(dbeta), _p(coef4), _p(gs), int(group), nb, C, P,
                                                 int(want_bound), _stream())
    torch.cuda.synchronize()
    return rc, partial, dgamma, dbeta, coef4, gs


@pytest.mark.parametrize("want_bound", [0, 1], ids=["nobound", "bound"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "%dx%dx%d-K%d" % s)
def test_reduce_wide(shape, relu, want_bound):
    from gemm_gpu_helpers import _logged
    nb, C, P, K = shape
    d = _case(shape)
    c = d.case
    assert c.band == 0
    r = bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu, group=K)
    (rc, partial, dgamma, dbeta, coef4, gsum), got = _logged(
        _lib(), lambda: _reduce_wide_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu, K, want_bound))
    assert rc == 0
    NP = math.ceil(K / 256)
    assert [w for _, w in got] == [nb * C, (C + 63) // 64] and "::bn_bwd_reduce_wide_kernel<%d>(" % NP in got[0][0] \
        and "::bn_bwd_finalize_kernel(" in got[1][0], got
    tag = "wide %dx%dx%d K%d %s" % (nb, C, P, K, "relu" if relu else "lin")
    g = host(gsum).astype(np.float64)
    _worst(tag + " gsum[0]", np.abs(g[0] - r.gsum[0]), (NP + 7) * U * r.gmag[0])
    _worst(tag + " gsum[1]", np.abs(g[1] - r.gsum[1]), (NP + 7) * U * r.gmag[1])
    assert tuple(partial.shape) == (3 if want_bound else 2, nb, C)
    _check_sums(tag, r, partial, dgamma, dbeta, coef4, d.coef, _row_lanes(P, K))
    if relu and c.zero.any():
        assert not host(partial)[:, :, c.zero].any(), "the zero channel's gate is closed: strict > 0"
    if want_bound:
        f = bo.finalize_partials_f64(host(dbeta), host(dgamma), nb * P, c.coef, c.mean, c.invstd, mx=r.mx.max(0))
        row4 = host(coef4)[4, :(C + 63) // 64].astype(np.float64)
        assert (np.abs(row4 - f.row4) <= 8 * U * f.row4).all(), (row4, f.row4)
    # the same bits on every run
    again = _reduce_wide_raw(d.dz, d.y, d.coef, d.mean, d.invstd, relu, K, want_bound)
    for a, b, what in zip(again[1:], (partial, dgamma, dbeta, coef4[:4], gsum), ("partial", "dgamma", "dbeta", "coef4", "gsum")):
        _same_bits(a[:4] if what == "coef4" else a, b, tag + " second run: " + what)
    # dgamma, dbeta and coef4 are what the finalisation from partial sums makes of the same partial
    fg, fb, fc = _ops().bn_backward_from_partials(partial[:2].contiguous(), nb * P, d.coef, d.mean, d.invstd)
    _same_bits(fg, dgamma, tag + " from partials: dgamma")
    _same_bits(fb, dbeta, tag + " from partials: dbeta")
    _same_bits(fc[:4], coef4[:4], tag + " from partials: coef4")
    # the wrapper gives the bits of the C entry
    out = _ops().bn_backward_reduce_wide(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, relu, K, want_bound=want_bound)
    for a, b, what in zip(out, (dgamma, dbeta, coef4, gsum), ("dgamma", "dbeta", "coef4", "gsum")):
        _same_bits(a[:4] if what == "coef4" else a, b[:4] if what == "coef4" else b, tag + " wrapper " + what)


def test_reduce_wide_refusals():
    """group 256 (the narrow entry's), 258 (no multiple of 4), 1028 (more than four passes), P % group != 0, plain mode, no gsum
    and a view that is not 16-B aligned are refused before anything is launched"""
    ops = _ops()
    shape = (1, 2, 3072)
    case = bo.build_case(bo.case_seed(*shape, "wide refuse"), *shape)
    d = _Dev(case)
    for group, P in ((256, 3072), (258, 2064), (1028, 2056)):
        assert P % group == 0 and P % 4 == 0 and P <= 3072
        with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_wide_f32"):
            ops.bn_backward_reduce_wide(d.dz[:, :, :P].contiguous(), d.y[:, :, :P].contiguous(), d.coef, d.mean, d.invstd,
                                        d.gamma, True, group)
    rc, partial, _, _, _, gsum = _reduce_wide_raw(d.dz, d.y, d.coef, d.mean, d.invstd, True, 448)      # 3072 % 448 != 0
    assert rc != 0 and bool(torch.isnan(partial).all()) and bool(torch.isnan(gsum).all()), "refused: nothing written"
    with pytest.raises(RuntimeError):
        ops.bn_backward_reduce_wide(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, True, 448)
    with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_wide_f32"):                         # plain: Y == NULL
        ops.bn_backward_reduce_wide(d.dz, None, d.coef, d.mean, d.invstd, d.gamma, True, 512)
    rc, partial, _, _, _, _ = _reduce_wide_raw(d.dz, d.y, d.coef, d.mean, d.invstd, True, 512, gsum=False)
    assert rc != 0 and bool(torch.isnan(partial).all()), "gsum is required"
    n = d.dz.numel()
    for which in ("dz", "y"):
        buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
        view = buf[1:1 + n].view(shape)
        view.copy_(getattr(d, which))
        args = (view, d.y) if which == "dz" else (d.dz, view)
        with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_wide_f32"):
            ops.bn_backward_reduce_wide(*args, d.coef, d.mean, d.invstd, d.gamma, True, 512)
    torch.cuda.synchronize()
    out = ops.bn_backward_reduce_wide(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, True, 512)         # and takes the aligned one
    assert tuple(out[3].shape) == (2, 1, 2, 6) and bool(torch.isfinite(out[3]).all())


def test_the_narrow_entry_still_refuses_a_wide_group():
    d = _case((1, 2, 2048, 512))
    with pytest.raises(RuntimeError, match="usip_bn_backward_reduce_f32"):
        _ops().bn_backward_reduce(d.dz, d.y, d.coef, d.mean, d.invstd, d.gamma, True, group=512)
