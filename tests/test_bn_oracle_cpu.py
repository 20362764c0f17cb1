"""What entitles tests/bn_oracle.py to judge the BatchNorm kernels (test_bn_kernels_gpu.py): its float64 sums and
coefficients against torch.nn.functional.batch_norm under double autograd, its forward statistics against numpy's, its
pooled form against the direct sparse sum -- and the conditions the GPU tests rely on, for the very inputs they build."""
import numpy as np
import pytest

import bn_oracle as bo


def _f64_coefficients(case):
    """(coef [4, C], mean, invstd) of the case's batch statistics in float64, nothing rounded to fp32"""
    y = bo.f64(case.y)
    mean = y.mean((0, 2))
    var = ((y - mean[None, :, None]) ** 2).mean((0, 2))
    invstd = 1.0 / np.sqrt(var + bo.EPS)
    sc = bo.f64(case.gamma) * invstd
    return np.stack([sc, bo.f64(case.beta) - mean * sc, mean, invstd]), mean, invstd


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", [(1, 6, 1), (5, 6, 1), (1, 6, 5), (4, 6, 1025)], ids=lambda s: "n%d" % (s[0] * s[2]))
def test_the_coefficient_form_is_autograds_gradient(shape, relu):
    """a1*dYhat + q1*y + q0 from reduce_f64's float64 coefficients == dY of F.batch_norm(+relu) in double, 1e-10 of
    max |dY| per channel; dgamma and dbeta at 1e-10 of their terms' magnitudes.  nb*P = 1 (var = 0, dY = 0), 5 and 4100;
    channels up to 90 deviations off centre, dZ scales 1e-6 .. 1e4, the zero channel and a gamma == 0 channel."""
    case = bo.build_case(bo.case_seed(*shape, "autograd"), *shape)
    assert case.band == 0
    ratio = np.abs(bo.f64(case.mean) * bo.f64(case.invstd))
    assert ratio.max() <= 100 and (shape[0] * shape[2] < 100 or ratio.max() > 30), ratio
    coef, mean, invstd = _f64_coefficients(case)
    r = bo.reduce_f64(case.dz, case.y, coef, mean, invstd, relu)
    dy, dgamma, dbeta = bo.dy_autograd_f64(case.y, case.gamma, case.beta, bo.EPS, relu, case.dz)
    form = bo.coef_form(r.coef4, r.dyh, case.y)
    per = np.abs(dy).max((0, 2))
    assert (np.abs(form - dy).max((0, 2)) <= 1e-10 * per).all(), np.abs(form - dy).max((0, 2)) / np.maximum(per, 1e-300)
    assert (np.abs(bo.dy_f64(r) - dy).max((0, 2)) <= 1e-10 * per).all()
    assert (np.abs(r.dgamma - dgamma) <= 1e-10 * r.H2.sum(0)).all()
    assert (np.abs(r.dbeta - dbeta) <= 1e-10 * r.H1.sum(0)).all()
    if shape[0] * shape[2] > 1:
        assert per[0] > 0
    # the bound the kernels write (row 4) holds for the true gradient, channel by channel
    assert (np.abs(dy).max((0, 2)) <= r.bound * (1 + 1e-12)).all()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_an_fp32_forward_mean_costs_more_than_the_coefficients_rounding(relu):
    """The conditioning input of the GPU file, no kernel: the float64 oracle on the fp32 forward statistics against autograd
    on the exact ones.  Without ReLU the difference is already 2.5 times coefficient_rounding_bar (so no kernel can be held
    to that bar against autograd), and it is inside that bar plus forward_mean_rounding_bar."""
    case = bo.build_case(bo.case_seed("conditioning"), *bo.CONDITIONING_SHAPE)
    r = bo.reduce_f64(case.dz, case.y, case.coef, case.mean, case.invstd, relu)
    dy, _, _ = bo.dy_autograd_f64(case.y, case.gamma, case.beta, bo.EPS, relu, case.dz)
    err = np.abs(bo.dy_f64(r) - dy)
    rounding = bo.coefficient_rounding_bar(r, case.y)
    wide = rounding + bo.forward_mean_rounding_bar(r)
    assert not err[wide == 0].any()
    alone = (err[rounding > 0] / rounding[rounding > 0]).max()
    both = (err[wide > 0] / wide[wide > 0]).max()
    print("oracle on fp32 statistics against autograd: %.3f of the 16 U bar, %.3f with the mean's term" % (alone, both))
    assert both <= 1.0
    if not relu:
        assert alone > 2.0
        ch = np.unravel_index(np.argmax(np.where(rounding > 0, err / np.maximum(rounding, 1e-300), 0)), err.shape)[1]
        assert abs(float(case.mean[ch]) * float(case.invstd[ch])) > 80 and abs(r.c2m[ch]) < 0.05 * abs(r.c1m[ch])


def test_the_gate_is_strict_and_zero_stays_closed():
    """relu_gate is `> 0` as torch's ReLU backward: an activation of exactly 0 (y == 0, shift == 0; or y*sc == -sh) is
    closed, and move_off_the_gate leaves such elements where they are."""
    y = bo.f32([[[0.0, 1.0, -1.0, 2.0]], [[0.0, 0.0, 0.0, 0.0]]]).transpose(1, 0, 2).copy()      # [1, 2, 4]
    sc, sh = bo.f32([1.0, 3.0]), bo.f32([-1.0, 0.0])
    gate = bo.relu_gate(y, sc, sh)
    assert gate.tolist() == [[[False, False, False, True], [False, False, False, False]]]
    moved, n = bo.move_off_the_gate(y, sc, sh, 1e-4)
    assert n == 0 and np.array_equal(moved, y)
    y2 = bo.f32([[[1.00001, 0.99999, 5.0]]])
    moved, n = bo.move_off_the_gate(y2, bo.f32([1.0]), bo.f32([-1.0]), 1e-4)
    assert n == 2 and moved[0, 0, 2] == 5.0 and not bo.gate_band(moved, [1.0], [-1.0], 1e-4).any()
    t = bo.f64(moved)[0, 0] - 1.0
    assert t[0] > 0 > t[1], "an element leaves the band on the side it was on"
    # torch agrees on the strict gate
    _, _, dbeta = bo.dy_autograd_f64(np.zeros((2, 1, 3)), [1.0], [0.0], bo.EPS, True, np.ones((2, 1, 3)))
    assert dbeta[0] == 0.0


@pytest.mark.parametrize("tiles", [1, 3, 257])
def test_finalize_of_exact_tile_sums_is_numpys_mean_and_variance(tiles):
    """partials that are exact in fp32 (y a multiple of 1/16 under 4: a tile of 8 sums exactly): finalize_f64's mean and
    biased variance are y.mean() and y.var() in float64, its unbiased factor n/(n-1), its running statistics the blend"""
    rng = np.random.default_rng(tiles)
    C, T = 3, 8
    y = rng.integers(-16, 17, (C, tiles, T)) / 16.0 + np.array([3.0, -2.0, 0.0])[:, None, None]
    stats = np.stack([y.sum(-1), (y * y).sum(-1)])
    assert np.array_equal(bo.f32(stats).astype(np.float64), stats)
    n = tiles * T
    gamma, beta = bo.f32([1.5, -0.5, 0.0]), bo.f32([0.1, 0.2, 0.3])
    rm, rv = bo.f32([1.0, 2.0, 3.0]), bo.f32([4.0, 5.0, 6.0])
    f = bo.finalize_f64(bo.f32(stats), n, gamma, beta, 1e-5, 0.1, rm, rv)
    flat = y.reshape(C, -1)
    assert np.allclose(f.mean, flat.mean(1), rtol=1e-14, atol=1e-15)
    assert np.allclose(f.var, flat.var(1), rtol=1e-11)
    m, e = float(np.float32(0.1)), float(np.float32(1e-5))
    assert np.allclose(f.invstd, 1 / np.sqrt(flat.var(1) + e), rtol=1e-11)
    assert np.allclose(f.coef[0], bo.f64(gamma) * f.invstd) and np.allclose(f.coef[1], bo.f64(beta) - f.mean * f.coef[0])
    assert np.array_equal(f.coef[2], f.mean) and np.array_equal(f.coef[3], f.invstd)
    assert np.allclose(f.running_mean, (1 - m) * bo.f64(rm) + m * flat.mean(1), rtol=1e-13)
    assert np.allclose(f.running_var, (1 - m) * bo.f64(rv) + m * flat.var(1, ddof=1), rtol=1e-11)
    g = bo.finalize_f64(bo.f32(stats), n, None, None, 1e-5, 0.1, None, None)
    assert np.array_equal(g.coef[0], g.invstd) and np.allclose(g.coef[1], -g.mean * g.invstd)
    assert g.running_mean is None and g.running_var is None


def test_finalize_of_one_sample_and_of_a_negative_variance():
    """count == 1: the unbiased factor is 1, not n/(n-1) = 1/0.  q/n < mean^2 (partials rounded apart): var clamps to 0"""
    stats = bo.f32([[[3.0]], [[9.0]]])
    f = bo.finalize_f64(stats, 1, None, None, 1e-5, 0.5, bo.f32([1.0]), bo.f32([1.0]))
    assert f.var[0] == 0 and np.isfinite(f.running_var).all() and f.running_var[0] == 0.5
    assert f.invstd[0] == 1 / np.sqrt(float(np.float32(1e-5)))
    f = bo.finalize_f64(bo.f32([[[6.0, 6.0]], [[17.0, 18.0]]]), 4, None, None, 1e-5, 0.5, None, None)     # q/n = 8.75 < 9
    assert f.var[0] == 0 and np.isfinite(f.coef).all()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 1), (2, 3, 7, 4), (1, 2, 33, 16)], ids=str)
def test_pool_scatter_then_reduce_is_the_direct_sparse_sum(shape, relu):
    case = bo.build_pool_case(*shape)
    nb, C, M, K = shape
    dense = bo.pool_scatter(case.dpooled, case.arg, K)
    assert dense.shape == (nb, C, M * K) and (dense != 0).sum() == (case.dpooled != 0).sum()
    assert np.array_equal(dense.reshape(nb, C, M, K)[0, 0, :, 0], case.dpooled[0, 0]), "first row: arg pinned at 0"
    assert np.array_equal(dense.reshape(nb, C, M, K)[-1, -1, :, K - 1], case.dpooled[-1, -1]), "last row: at K - 1"
    r = bo.reduce_f64(dense, case.y, case.coef, case.mean, case.invstd, relu)
    s1 = np.zeros((nb, C))
    s2 = np.zeros((nb, C))
    for b in range(nb):
        for c in range(C):
            for m in range(M):
                yv = float(case.y[b, c, m * K + case.arg[b, c, m]])
                assert yv == float(case.yarg[b, c, m])
                t = np.float32(yv * float(case.coef[0, c]) + float(case.coef[1, c]))
                d = float(case.dpooled[b, c, m]) if (not relu or t > 0) else 0.0
                s1[b, c] += d
                s2[b, c] += d * (yv - float(case.mean[c])) * float(case.invstd[c])
    assert (np.abs(r.s1 - s1) <= 1e-13 * r.H1).all() and (np.abs(r.s2 - s2) <= 1e-13 * r.H2).all()


def test_group_sums_add_up_to_the_row_sums():
    case = bo.build_case(bo.case_seed(2, 3, 48, "group"), 2, 3, 48)
    r = bo.reduce_f64(case.dz, case.y, case.coef, case.mean, case.invstd, True, group=8)
    assert r.gsum.shape == (2, 2, 3, 6)
    assert np.allclose(r.gsum[0].sum(-1), r.s1, rtol=1e-13, atol=0) or (np.abs(r.gsum[0].sum(-1) - r.s1) <= 1e-13 * r.H1).all()
    assert np.allclose(r.gsum[1].sum(-1), bo.f64(case.y).sum(-1), rtol=1e-12)
    assert (r.gmag[0] >= np.abs(r.gsum[0])).all() and (r.gmag[1] >= np.abs(r.gsum[1]) * (1 - 1e-15)).all()
    assert np.array_equal(r.row4, [r.bound.max()])


@pytest.mark.parametrize("name,thunk", bo.all_builders(), ids=[n for n, _ in bo.all_builders()])
def test_every_gpu_input_is_off_the_gate(name, thunk):
    """A CONDITION of the GPU tests, not a measurement: after move_off_the_gate no element of any input they build lies
    within 1e-4 * (|y*sc| + |sh|) of the gate, fewer than 1 % of the elements were moved for it, and |mu| * is <= 100.
    The seeds (bn_oracle.case_seed) were picked so that this holds."""
    case = thunk()
    assert case.band == 0, "%s: %d elements left in the band" % (name, case.band)
    assert case.moved < 0.01 * case.y.size, "%s: %d of %d moved" % (name, case.moved, case.y.size)
    assert (np.abs(bo.f64(case.mean) * bo.f64(case.invstd)) <= 100).all()
    assert np.isfinite(case.y).all() and np.isfinite(case.dz).all() and np.isfinite(case.coef).all()
    # the statistics are those of the final y
    mean, invstd, coef = bo.forward_coefficients(case.y, case.gamma, case.beta)
    assert np.array_equal(mean, case.mean) and np.array_equal(invstd, case.invstd) and np.array_equal(coef, case.coef)
    # the special channels are what the GPU tests take them for
    if case.zero.any():
        assert not case.y[:, case.zero].any() and not case.coef[1, case.zero].any()
    if case.gamma0.any():
        assert not case.coef[0, case.gamma0].any()


def test_the_dense_cases_reach_every_loop_tail():
    """the list of dense shapes holds every P, C and nb at which a loop of the reduce or finalize kernels takes another turn,
    each of them at least once"""
    nbs, Cs, Ps = ({c[i] for c in bo.DENSE_CASES} for i in range(3))
    assert {1, 2, 3, 4, 8, 1020, 1024, 1028, 2052, 4100} <= Ps
    assert {1, 63, 64, 65, 130} <= Cs and {1, 7, 8, 9, 17} <= nbs
    assert all(nb * C * P < 2_000_000 for nb, C, P, _ in bo.DENSE_CASES)
    assert len(bo.group_cases()) == 28 and all(P % K == 0 for _, _, P, K in bo.group_cases())


@pytest.mark.parametrize("rows", [1, 2, 15, 17, 1000])
def test_cancelling_partials_cancel_exactly_in_double(rows):
    p = bo.cancelling_partials(rows, rows, 5)
    assert p.shape == (2, rows, 5) and p.dtype == np.float32
    exact = np.array([[float(sum(int(v * 16) for v in p[k, :, c])) / 16 for c in range(5)] for k in range(2)])
    for order in (np.arange(rows), np.arange(rows)[::-1], np.random.default_rng(0).permutation(rows)):
        acc = np.zeros((2, 5))
        for i in order:
            acc += p[:, i].astype(np.float64)
        assert np.array_equal(acc, exact)
    assert np.abs(exact).max() <= 2.0 * ((rows + 1) // 2)
    if rows > 1:
        assert np.abs(p).max() >= 0.5e6
        chain = np.zeros((2, 5), np.float32)
        for i in range(rows):
            chain += p[:, i]
        assert rows < 15 or (chain.astype(np.float64) != exact).any(), "an fp32 chain would lose these"
