"""tests/segment_oracle.py on the CPU alone: its exactness assertions hold for every fixture, every fixture still covers the
path it exists for (the claims against their floors), its checker refuses wrong segments, and the oracle itself agrees with
torch -- scatter_add_, gather + cat + conv1d, softplus, Adam -- and with the reference's index_max host twin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import segment_oracle as so


def test_cumsum_in_float32_is_the_sequential_chain():
    """what segment_sum_listorder stands on: ((r0 + r1) + r2) + ..., not numpy's pairwise sum"""
    r = np.random.default_rng(0).standard_normal(4099).astype(np.float32)
    acc, chain = np.float32(0), []
    for x in r:
        acc = acc + x
        chain.append(acc)
    assert np.array_equal(so.bits(np.cumsum(r, dtype=np.float32)), so.bits(np.asarray(chain)))
    assert np.float32(r.sum()) != chain[-1]                                 # and the order matters for these values
    src = r[None, None, :]
    start, perm = np.asarray([[0, 0, 4099]], np.int32), np.arange(4099, dtype=np.int32)[None, ::-1].copy()
    back = np.float32(0)
    for x in r[::-1]:
        back = back + x
    assert so.bits(so.segment_sum_listorder(src, start, perm, 1))[0, 0].tolist() == [0, so.bits(back)[()]]


def _cpu_perm(idx, N):
    start = so.csr_start(idx, N)
    perm = np.zeros(idx.shape, np.int32)
    for b in range(idx.shape[0]):
        valid = np.flatnonzero((idx[b] >= 0) & (idx[b] < N))
        perm[b, :len(valid)] = valid[np.argsort(idx[b][valid], kind="stable")]
    return start, perm


def test_the_checker_accepts_a_sorted_perm_and_refuses_wrong_ones():
    rng = np.random.default_rng(1)
    N, P = 9, 700
    idx = np.stack([so.idx_of_lengths(rng, (0, 1, 3, 4, 5, 7, 8), N, P, junk=6) for _ in range(2)])
    claims = so.segment_claims(idx, N)
    assert claims["junk"] == 12 and claims["empty"] == 1 and {0, 1, 3, 4, 5, 7, 8} <= claims["lengths"]
    start, perm = _cpu_perm(idx, N)
    assert so.check_perm(idx, N, start, perm) == 2 * N
    s0, s1 = int(start[1, 8]), int(start[1, 9])
    assert s1 - s0 > 200
    inside = perm.copy()                                                    # any order inside one 64-position block passes
    seg = inside[1, s0:s1]
    first = np.flatnonzero(seg // 64 == seg[0] // 64)
    seg[first] = seg[first][::-1]
    if len(first) > 1:
        so.check_perm(idx, N, start, inside)
    for wrong in ("cell", "block", "junk", "twice", "start"):
        st, pm = start.copy(), perm.copy()
        if wrong == "cell":
            pm[1, [s0 - 1, s0]] = pm[1, [s0, s0 - 1]]
        elif wrong == "block":
            pm[1, [s0, s1 - 1]] = pm[1, [s1 - 1, s0]]
        elif wrong == "junk":
            pm[0, 3] = np.flatnonzero(idx[0] < 0)[0]
        elif wrong == "twice":
            pm[0, s0 + 1] = pm[0, s0]
        else:
            st[0, 4] += 1
        with pytest.raises(AssertionError):
            so.check_perm(idx, N, st, pm)


def test_segment_sums_equal_scatter_add():
    rng = np.random.default_rng(2)
    B, C, N, P = 2, 3, 40, 515
    idx = rng.integers(0, N, (B, P)).astype(np.int32)
    src = so.dyadic(rng, (B, C + 2, P), 4, 8)
    start, perm = _cpu_perm(idx, N)
    ref = torch.zeros(B, C, N, dtype=torch.float64)
    ref.scatter_add_(2, torch.from_numpy(idx).long().view(B, 1, P).expand(B, C, P), torch.from_numpy(src[:, 1:1 + C]).double())
    assert np.array_equal(so.segment_sum64(src, idx, C, N, 1), ref.numpy())
    assert np.array_equal(so.segment_sum_listorder(src, start, perm, C, 1).astype(np.float64), ref.numpy())   # dyadic: exact


@pytest.mark.parametrize("name", sorted(so.KNN_CASES))
def test_knn_fixtures_are_exact_and_cover_their_paths(name):
    c = so.knn_case(name)
    assert so.knn_claims_hold(name, c["claims"]), c["claims"]
    Y, d, n = so.knn_forward(c["U"], c["W"], c["database"], c["query"], c["idx"])      # asserts every step exact
    B, Cout, N = c["U"].shape
    _, M, K = c["idx"].shape
    P = M * K
    # torch.gather + cat + conv1d in float64 (models/layers.py:422-431): the coordinate columns and an identity on U
    flat = torch.from_numpy(n).view(B, 1, P)
    dt = torch.gather(torch.from_numpy(c["database"]).double(), 2, flat.expand(B, 3, P)) - \
        torch.from_numpy(c["query"]).double().repeat_interleave(K, dim=2)
    ut = torch.gather(torch.from_numpy(c["U"]).double(), 2, flat.expand(B, Cout, P))
    W = torch.cat([torch.from_numpy(c["W"][:, :3]).double(), torch.eye(Cout, dtype=torch.float64)], dim=1)
    ref = F.conv1d(torch.cat([dt, ut], dim=1), W.unsqueeze(2))
    assert np.array_equal(Y.astype(np.float64), ref.numpy()) and np.array_equal(d.astype(np.float64), dt.numpy())
    for relu in (False, True):
        g = so.knn_backward_g(c["dZ"], c["Yb"], c["coef4"], relu)
        so.knn_dwc_terms(g, d)
        cf = torch.from_numpy(c["coef4"]).double().view(4, 1, Cout, 1)
        y, dz = torch.from_numpy(c["Yb"]).double(), torch.from_numpy(c["dZ"]).double()
        dyh = torch.where(y * cf[0] + cf[1] > 0, dz, torch.zeros_like(dz)) if relu else dz
        assert np.array_equal(g.astype(np.float64), (cf[0] * dyh + cf[2] * y + cf[3]).numpy())
    terms = so.knn_stats(Y)
    small = P <= 4100
    for t, step in ((terms[0], 4), (terms[1], 8), (so.knn_dwc_terms(g, d), 8)):
        assert not small or so.any_order_exact(t, step).all(), name         # the small cases are held to bit patterns


@pytest.mark.parametrize("name", sorted(so.NODEMAX_CASES))
def test_node_max_fixtures_and_the_host_twin(name):
    from usip_amd import ops
    c = so.nodemax_case(name)
    assert so.nodemax_claims_hold(name, c["claims"]), c["claims"]
    C, K = c["C"], c["K"]
    B, Ctot, N = c["data"].shape
    mi, val = so.index_max_values(c["data"], c["index"], c["count"], K, C)
    twin = ops.index_max_cpu(torch.from_numpy(np.ascontiguousarray(c["data"][:, :C])), torch.from_numpy(c["index"]), K)
    assert np.array_equal(mi, twin.numpy())
    g = torch.from_numpy(c["data"][:, :C]).gather(2, torch.from_numpy(mi).long()) * torch.from_numpy(c["count"] > 0).float().unsqueeze(1)
    same = ~np.isnan(g.numpy())                                             # (NaN * 0 of an empty node is NaN there, +0.0 here)
    assert np.array_equal(val[same], g.numpy()[same]) and not np.isnan(val[same]).any()   # gather * mask, numerically
    # both backwards against index_add_ in float64
    ref = torch.from_numpy(c["src"][:, 1:1 + C]).double().clone()
    has = torch.from_numpy(c["count"] > 0)
    for b in range(B):
        for ch in range(C):
            ref[b, ch].index_add_(0, torch.from_numpy(mi[b, ch]).long()[has[b]], torch.from_numpy(c["g"][b, ch]).double()[has[b]])
    assert np.array_equal(so.index_max_scatter(c["g"], mi, c["count"], N, c["src"][:, 1:1 + C]).astype(np.float64), ref.numpy())
    assert c["index"].min() >= 0 and c["index"].max() < K                   # the kernel does not guard it


def test_softplus_rigid_loss_and_adam_agree_with_torch():
    x = np.concatenate([np.asarray(so.SIGMA_RAW, np.float32), np.linspace(-40, 40, 161, dtype=np.float32)]).astype(np.float64)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = F.softplus(xt)
    y.sum().backward()
    assert np.allclose(so.softplus64(x), y.detach().numpy(), rtol=1e-15, atol=0)
    assert np.allclose(so.softplus_grad64(x), xt.grad.numpy(), rtol=1e-15, atol=1e-300)
    assert so.softplus64(np.float32(20.000002)) == np.float32(20.000002) and so.softplus64(20.0) > 20.0

    rng = np.random.default_rng(3)
    B, M = 3, 17
    xx, R = so.dyadic(rng, (B, 3, M), 4, 8), so.dyadic(rng, (B, 3, 3), 2, 1)
    scale, shift = np.asarray([0.5, 1.5, -1.25], np.float32), so.dyadic(rng, (B, 3), 4, 4)
    Rs = torch.from_numpy(R).double() * torch.from_numpy(scale).double().view(B, 1, 1)
    ref = torch.baddbmm(torch.from_numpy(shift).double().unsqueeze(2), Rs, torch.from_numpy(xx).double())
    assert np.array_equal(so.rigid(xx, R, scale, shift).astype(np.float64), ref.numpy())
    assert np.array_equal(so.rigid(xx, R, scale, None, True).astype(np.float64),
                          torch.bmm(Rs.transpose(1, 2), torch.from_numpy(xx).double()).numpy())

    d = np.abs(so.dyadic(rng, (2, 1025), 6, 8))
    want = so.loss_combine64(d, 1.25, 0.75)
    dt = torch.from_numpy(d).double()
    assert np.allclose(want, [1.25 + 0.75 * (dt[0].mean() + dt[1].mean()), 0.75 * dt[0].mean(), 0.75 * dt[1].mean()], rtol=1e-15)
    assert np.allclose(so.loss_combine_steps(d, 1.25, 0.75), want, rtol=3 * 2.0 ** -24)

    n = 37
    p0, grads = rng.standard_normal(n), rng.standard_normal((3, n)) * 0.1
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False, fused=False)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        param.grad = torch.from_numpy(grads[t - 1].copy())
        opt.step()
        p, m, v = so.adam64(p, grads[t - 1], m, v, t, 1e-3, 0.9, 0.999, 1e-8, as_kernel=False)
        assert np.allclose(p, param.detach().numpy(), rtol=1e-13, atol=0)
        assert np.allclose(m, opt.state[param]["exp_avg"].numpy(), rtol=1e-13, atol=1e-300)
        assert np.allclose(v, opt.state[param]["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-300)
    pk, _, _ = so.adam64(p0, grads[0], np.zeros(n), np.zeros(n), 1, 1e-3, 0.9, 0.999, 1e-8)    # the kernel's float32 inputs
    p1, _, _ = so.adam64(p0, grads[0], np.zeros(n), np.zeros(n), 1, 1e-3, 0.9, 0.999, 1e-8, as_kernel=False)
    assert np.allclose(pk, p1, rtol=1e-9)
