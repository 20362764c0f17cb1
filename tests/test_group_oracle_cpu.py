"""CPU tests of tests/group_oracle.py: what entitles the GPU tests of the grouping and pooling kernels
(test_group_kernels_gpu.py) to use it as the checker.  The oracle's first-index max is torch.max(dim=3)'s on CPU tensors --
the first NaN, the first of -0.0 / +0.0, index 0 of a row of -inf -- its gather and scatter-add are torch.gather and
scatter_add_, its activation is torch's float32 arithmetic; every builder's claim holds at the seeds the GPU tests use."""
import numpy as np
import pytest
import torch

import group_oracle as go


def _same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(go.bits(a)[~np.isnan(a)], go.bits(b)[~np.isnan(b)])


def _torch_max(z):
    v, i = torch.max(torch.from_numpy(np.ascontiguousarray(z)), dim=-1)
    return v.numpy(), i.numpy().astype(np.int32)


def test_torch_cpu_max_rule_is_pinned_on_hand_written_rows():
    nan, inf = np.nan, np.inf
    z = np.asarray([[nan, 1, nan, 9], [1, nan, 5, nan], [-0.0, 0.0, -1, 0.0], [0.0, -0.0, -1, -0.0], [-inf] * 4,
                    [3, inf, inf, 3], [2, 2, 2, 2], [1, 7, 7, nan]], np.float32)
    want_arg = [0, 1, 0, 0, 0, 1, 0, 3]
    for pooled, arg in (_torch_max(z), go.first_max(z)):
        assert arg.tolist() == want_arg
        assert np.isnan(pooled[[0, 1, 7]]).all() and pooled[4] == -inf and pooled[5] == inf
        assert np.signbit(pooled[2]) and not np.signbit(pooled[3]) and pooled[2] == 0 and pooled[3] == 0


@pytest.mark.parametrize("K", go.GROUP_MAX_K)
def test_first_max_is_torch_max_on_every_row_kind(K):
    R = go.ragged_rows(K, go.SPECIAL_ROWS)
    z = np.concatenate([go.pool_case(K, R)[0], go.nan_rows(K)[0]])
    pooled, arg = go.first_max(z)
    tp, ta = _torch_max(z)
    assert np.array_equal(arg, ta) and _same(pooled, tp)
    assert _same(pooled, z[np.arange(len(z)), arg])
    sp = go.special_rows(K)
    p, a = go.first_max(sp)
    assert a[0] == 0 and p[0] == -np.inf and a[1] == K // 3 and p[1] == np.inf and a[5] == 0
    assert a[2] == a[3] == a[4] == K // 3 and p[2] == 0 and p[3] == 0
    assert np.signbit(p[2]) and not np.signbit(p[3]) and p[4] == np.float32(9 * 2.0 ** -149)


@pytest.mark.parametrize("K", go.GROUP_MAX_K)
def test_pool_rows_hold_their_claims(K):
    R = go.ragged_rows(K, go.SPECIAL_ROWS)
    z, claims = go.pool_case(K, R)
    assert z.shape == (R, K) and R >= K + go.SPECIAL_ROWS and R % 2 == 1
    assert go.pool_claims_hold(K, claims), (K, claims, go.POOL_FLOORS[K])
    assert np.array_equal(np.argmax(z[:K], axis=1), np.arange(K))           # the rotating maximum
    ties = z[:R - go.SPECIAL_ROWS]
    assert np.array_equal(ties * 64, np.rint(ties * 64)) and np.abs(ties).max() <= 8
    assert np.array_equal(go.bits(z[R - go.SPECIAL_ROWS:]), go.bits(go.special_rows(K)))
    for small in (1, 3):
        zs, _ = go.pool_case(K, small)
        assert zs.shape == (small, K)
    fam, L = go.max_kernel_of(K)
    per = 4 * (256 // L) if fam == "max4" else 256 // L
    assert 0 < R % per < per
    if fam == "max4":                                                       # thread groups with one and with two rows
        assert 256 // L < R % per < 2 * (256 // L)
        assert R % (256 // go.max_kernel_of(K, aligned=False)[1]) != 0      # and the scalar kernel ends ragged too


def test_every_instantiation_is_reached_by_the_k_list():
    reached = {go.max_kernel_of(K) for K in go.GROUP_MAX_K}
    reached |= {go.max_kernel_of(K, aligned=False) for K in go.GROUP_MAX_K if K % 4 == 0}
    assert {("max4", L) for L in (1, 2, 4, 8, 16, 32, 64)} <= reached
    assert {("max", L) for L in (1, 2, 4, 8, 16, 32, 64)} <= reached
    assert {go.max_kernel_of(K) for K in go.ACT_K} == {("max4", L) for L in (1, 2, 4, 8, 16, 32, 64)}
    assert go.max_kernel_of(12) == ("max", 16) and go.max_kernel_of(512) == ("max", 64)
    assert go.max_kernel_of(16, aligned=False) == ("max", 16) and go.max_kernel_of(64, aligned=False) == ("max", 64)


@pytest.mark.parametrize("K", (16, 256))
def test_nan_rows_hold_their_claims(K):
    z, claims = go.nan_rows(K)
    first, behind, two = go.nan_floors(K)
    assert claims["first"] == first and claims["behind"] >= behind and claims["two"] >= two, claims
    pooled, arg = go.first_max(z)
    assert np.isnan(pooled).all() and np.array_equal(arg, np.argmax(np.isnan(z), axis=1))
    assert np.array_equal(arg[:K], np.arange(K))
    if K == 16:                                                             # the example of group.hip's header
        assert np.isnan(z[2, 2]) and z[2, 10] == 7.5 and np.nanmax(z[2]) == 7.5


def test_activation_is_exact_and_is_torchs_float32():
    for K in go.ACT_K:
        for shape in go.ACT_SHAPES:
            B, C, M = shape
            y, coef, claims = go.act_case(go.act_seed(B, C, M, K), B, C, M, K)
            assert go.act_claims_hold(shape, claims), (K, shape, claims)
            assert np.isnan(coef[2:]).all() and len(set(coef[0].tolist())) == C
            assert np.array_equal(y * 64, np.rint(y * 64)) and np.array_equal(coef[1] * 16, np.rint(coef[1] * 16))
            assert not np.signbit(coef[1][coef[1] == 0]).any()
            ty, tc = torch.from_numpy(y), torch.from_numpy(coef)
            for relu in (False, True):
                t = ty * tc[0].view(1, C, 1, 1) + tc[1].view(1, C, 1, 1)
                t = torch.relu(t) if relu else t
                a = go.act(y, coef, relu)
                assert np.array_equal(go.bits(a), go.bits(t.numpy()))
                pooled, arg, yarg = go.max_act(y, coef, relu)
                tp, ta = torch.max(t, dim=3)
                assert np.array_equal(arg, ta.numpy()) and np.array_equal(go.bits(pooled), go.bits(tp.numpy()))
                assert np.array_equal(go.bits(yarg), go.bits(torch.gather(ty, 3, ta.unsqueeze(3)).squeeze(3).numpy()))
            if C >= 3:
                assert (go.act(y, coef, True)[:, 2] == 0).all() and (go.max_act(y, coef, True)[1][:, 1:3] == 0).all()
                assert np.array_equal(go.max_act(y, coef, False)[1][:, 0], np.argmin(y[:, 0], axis=2))


def test_activation_turns_nan_into_zero_under_relu_only():
    y = np.asarray([[[[1.0, np.nan, -2.0, 0.5]]]], np.float32)
    coef = np.asarray([[1.0], [-1.0]], np.float32)
    assert go.max_act(y, coef, True)[1].tolist() == [[[0]]] and go.max_act(y, coef, True)[0].tolist() == [[[0.0]]]
    pooled, arg, yarg = go.max_act(y, coef, False)
    assert np.isnan(pooled).all() and arg.tolist() == [[[1]]] and np.isnan(yarg).all()


@pytest.mark.parametrize("name", sorted(go.GATHER_CASES))
def test_gather_is_torch_gather(name):
    x, idx, sub, coff, Ctot, want = go.gather_case(name)
    B, C, N = x.shape
    _, M, K = idx.shape
    flat = torch.from_numpy(idx).long().view(B, 1, M * K).expand(B, C, M * K)
    ref = torch.gather(torch.from_numpy(x), 2, flat).view(B, C, M, K).clone()
    if sub is not None:
        ref[:, :sub.shape[1]] -= torch.from_numpy(sub).unsqueeze(3)
    assert np.array_equal(go.bits(want[:, coff:coff + C]), go.bits(ref.numpy()))
    outside = np.delete(want, np.arange(coff, coff + C), axis=1)
    assert outside.size > 0 and (outside == go.SENTINEL).all() and coff > 0 and Ctot > coff + C
    assert (idx[:, 0, 0] == 0).all() and (idx[:, -1, -1] == N - 1).all()


@pytest.mark.parametrize("name", sorted(go.GATHER_BWD_CASES))
def test_scatter_add_is_torch_scatter_add_and_holds_its_claims(name):
    dout, idx, C, N, coff, want, claims = go.gather_bwd_case(name)
    assert go.scatter_claims_hold(name, claims), (name, claims)
    B, Ctot, M, K = dout.shape
    assert coff > 0 and Ctot > coff + C and C % 2 == 1
    assert np.isnan(dout[:, :coff]).all() and np.isnan(dout[:, coff + C:]).all() and not np.isnan(dout[:, coff:coff + C]).any()
    flat = torch.from_numpy(idx).long().view(B, 1, M * K).expand(B, C, M * K)
    src = torch.from_numpy(dout[:, coff:coff + C].reshape(B, C, M * K)).double()
    ref = torch.zeros(B, C, N, dtype=torch.float64).scatter_add_(2, flat, src)
    assert np.array_equal(want.astype(np.float64), ref.numpy()) and not np.signbit(want[want == 0]).any()
    named = np.zeros((B, N), bool)
    for b in range(B):
        named[b, idx[b].reshape(-1)] = True
    assert (want.transpose(0, 2, 1)[~named] == 0).all()


def test_dyadic_gradients_sum_exactly_in_float32_in_any_order():
    rng = np.random.default_rng(5)
    g = go.dyadic(rng, 4096, 4, 8)
    exact = float(g.astype(np.float64).sum())
    for _ in range(4):
        acc = np.float32(0)
        for v in rng.permutation(g):
            acc = np.float32(acc + v)
        assert float(acc) == exact


def test_pool_backwards_are_a_scatter_and_one_float32_add():
    rng = np.random.default_rng(6)
    K = 12
    dp = go.dyadic(rng, (2, 3, 5), 4, 8)
    dp[0, 0, :3] = [np.inf, np.nan, -0.0]
    arg = rng.integers(0, K, (2, 3, 5)).astype(np.int32)
    dz = go.max_backward(dp, arg, K)
    ref = torch.zeros(2, 3, 5, K).scatter_(3, torch.from_numpy(arg).long().unsqueeze(3), torch.from_numpy(dp).unsqueeze(3))
    assert np.array_equal(go.bits(dz), go.bits(ref.numpy()))
    assert (go.bits(dz) != 0).sum() <= dp.size                              # every other slot is +0.0
    base = rng.normal(0, 1, (2, 3, 5, K)).astype(np.float32)
    got = go.max_backward_add(base, dp, arg)
    want = torch.from_numpy(base).clone()
    want.scatter_add_(3, torch.from_numpy(arg).long().unsqueeze(3), torch.from_numpy(dp).unsqueeze(3))
    nan = np.isnan(got)
    assert np.array_equal(nan, np.isnan(want.numpy())) and np.array_equal(go.bits(got)[~nan], go.bits(want.numpy())[~nan])
    assert (go.bits(got) != go.bits(base)).sum() <= dp.size
