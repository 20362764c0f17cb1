"""The grouping and pooling kernels (csrc/group.hip) against tests/group_oracle.py on every dispatch path, bit for bit: the
inputs are dyadic (see the oracle), so nothing rounds and every check is on bit patterns.

Which case reaches which kernel:
  group_gather_bwd_lds_kernel<2, true>    N <= 2048, P % 4 == 0, aligned: n40_p4, n40_p20, n40_p1028(_one), n2048_p20, n2048_p1028
                                          (N = 2048: exactly 64 KiB of dynamic LDS)
  group_gather_bwd_lds_kernel<2, false>   n1_p1, n40_p3 (P % 4 != 0); n40_p1028 / n40_p20 / n2048_p1028 with dout or idx one
                                          element into a larger buffer (contiguous, not 16-byte aligned)
  group_gather_bwd_kernel (atomics)       n2049_p1, n2049_p1028 (the first atomic launch), n4096_p1028(_one); M = 0 stops
                                          after the memset
  group_max4_kernel<1..64>                K = 4, 8, 16, 32, 64, 128, 256 (ops.group_max on an aligned z, and ops.group_max_act)
  group_max_kernel<1, 2, 4, 8, 16, 32>    K = 1, 2, 3 (and 4 misaligned), 5 (8), 12 (16), 20 (32)
  group_max_kernel<64>                    K = 65, 100, 260, 512, and K = 64, 128, 256 through the view offset by 4 bytes
  group_max_bwd4_kernel / _bwd_kernel     K % 4 == 0 / the others of the same list
Every row count is 1, 3 and group_oracle.ragged_rows: a partly filled last workgroup, and thread groups of the vector kernel
with one and with two of their four rows."""
import ctypes

import numpy as np
import pytest
import torch

import group_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _off4(a):
    """the same values in a contiguous view that starts 4 bytes into a larger buffer: not 16-byte aligned"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _bits(t):
    return go.bits(t.detach().cpu().numpy())


def _same(got, want):
    """bit for bit where want is a number; NaN where want is NaN"""
    got, want = got.detach().cpu().numpy(), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(go.bits(got)[~nan], go.bits(want)[~nan])


# ----------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("name", sorted(go.GATHER_CASES))
def test_gather_writes_its_channel_slice_and_nothing_else(name):
    from usip_amd import ops
    x, idx, sub, coff, Ctot, want = go.gather_case(name)
    B, C, N = x.shape
    out = torch.full(want.shape, float(go.SENTINEL), device=DEV)
    ops.group_gather(_dev(x), _dev(idx), sub=None if sub is None else _dev(sub), out=out, coff=coff)
    assert Ctot > coff + C and coff > 0
    assert np.array_equal(_bits(out), go.bits(want))
    assert (out[:, :coff] == float(go.SENTINEL)).all() and (out[:, coff + C:] == float(go.SENTINEL)).all()
    alone = ops.group_gather(_dev(x), _dev(idx), sub=None if sub is None else _dev(sub))
    assert np.array_equal(_bits(alone), go.bits(want[:, coff:coff + C]))


def _gather_backward(dout, idx, C, N, coff):
    """the C entry point on a dx that holds NaN (ops.group_gather_backward hands it torch.empty)"""
    from usip_amd import _lib
    B, Ctot, M, K = dout.shape
    dx = torch.full((B, C, N), float("nan"), device=DEV)
    stream = torch.cuda.current_stream(dx.device).cuda_stream
    rc = _lib.lib().usip_group_gather_backward_f32(
        ctypes.c_void_p(dout.data_ptr()), ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(dx.data_ptr()),
        B, C, N, M, K, Ctot, coff, ctypes.c_void_p(stream))
    _lib.check(rc, "usip_group_gather_backward_f32")
    return dx


GATHER_BWD_RUNS = [(n, "aligned") for n in sorted(go.GATHER_BWD_CASES)] + [
    ("n40_p1028", "dout"), ("n40_p1028", "idx"), ("n40_p20", "dout"), ("n40_p20", "idx"), ("n2048_p1028", "idx"),
    ("n2048_p1028", "dout"), ("n4096_p1028", "dout")]


@pytest.mark.parametrize("name,offset", GATHER_BWD_RUNS)
def test_gather_backward_equals_the_exact_scatter_add(name, offset):
    dout, idx, C, N, coff, want, claims = go.gather_bwd_case(name)
    assert go.scatter_claims_hold(name, claims), (name, claims)
    d = _off4(dout) if offset == "dout" else _dev(dout)
    i = _off4(idx) if offset == "idx" else _dev(idx)
    assert d.data_ptr() % 16 == (4 if offset == "dout" else 0) and i.data_ptr() % 16 == (4 if offset == "idx" else 0)
    dx = _gather_backward(d, i, C, N, coff)
    assert np.array_equal(_bits(dx), go.bits(want))                         # a point nobody names: +0.0, not NaN
    if N <= 2048:                                                           # the LDS kernels: the same bits on every launch
        for _ in range(20):
            assert torch.equal(_gather_backward(d, i, C, N, coff), dx)


def test_gather_backward_of_no_positions_is_all_zeros():
    B, C, N, K = 2, 3, 40, 4
    dout = torch.full((B, C + 2, 0, K), float("nan"), device=DEV)
    idx = torch.zeros((B, 0, K), dtype=torch.int32, device=DEV)
    dx = _gather_backward(dout, idx, C, N, 1)
    assert not _bits(dx).any()


# ----------------------------------------------------------------------------------------------- max over K
@pytest.mark.parametrize("K", go.GROUP_MAX_K)
def test_group_max_equals_the_first_index_max(K):
    from usip_amd import ops
    ragged = go.ragged_rows(K, go.SPECIAL_ROWS)
    assert go.pool_claims_hold(K, go.pool_case(K, ragged)[1]), (K, go.pool_case(K, ragged)[1])
    for R in (1, 3, ragged):
        z, _ = go.pool_case(K, R)
        want, want_arg = go.first_max(z)
        views = [_dev(z).view(1, 1, R, K)] + ([_off4(z).view(1, 1, R, K)] if K % 4 == 0 else [])
        for v in views:
            pooled, arg = ops.group_max(v)
            assert np.array_equal(arg.cpu().numpy().reshape(-1), want_arg), (K, R, v.data_ptr() % 16)
            assert np.array_equal(_bits(pooled).reshape(-1), go.bits(want)), (K, R, v.data_ptr() % 16)


@pytest.mark.parametrize("K", go.ACT_K)
def test_group_max_act_equals_the_activated_first_index_max(K):
    from usip_amd import ops
    for shape in go.ACT_SHAPES:
        B, C, M = shape
        y, coef, claims = go.act_case(go.act_seed(B, C, M, K), B, C, M, K)
        assert go.act_claims_hold(shape, claims), (K, shape, claims)
        assert coef.shape == (4, C) and np.isnan(coef[2:]).all()
        yd, cd = _dev(y), _dev(coef)
        for relu in (False, True):
            want, want_arg, want_yarg = go.max_act(y, coef, relu)
            pooled, arg, yarg = ops.group_max_act(yd, cd, relu, want_yarg=True)
            pooled2, arg2 = ops.group_max_act(yd, cd, relu)
            for p, a in ((pooled, arg), (pooled2, arg2)):
                assert np.array_equal(a.cpu().numpy(), want_arg), (K, shape, relu)
                assert np.array_equal(_bits(p), go.bits(want)), (K, shape, relu)
            assert np.array_equal(_bits(yarg), go.bits(want_yarg)), (K, shape, relu)


def test_group_max_act_refuses_what_it_has_no_kernel_for():
    from usip_amd import ops
    coef = _dev(np.asarray([[1.0, 0.5], [0.0, 0.25]], np.float32))
    for K in (12, 512):
        with pytest.raises(RuntimeError):
            ops.group_max_act(torch.zeros(1, 2, 3, K, device=DEV), coef, True)
    with pytest.raises(RuntimeError):
        ops.group_max_act(_off4(np.zeros((1, 2, 3, 16), np.float32)), coef, True)
    pooled, arg = ops.group_max_act(torch.zeros(1, 2, 3, 16, device=DEV), coef, True)   # and takes the aligned one
    assert pooled.cpu().tolist() == [[[0.0] * 3, [0.25] * 3]] and not arg.any()


# ----------------------------------------------------------------------------------------------- its backwards
def _backward_case(K):
    """rows = 3 (K + 5): arg sweeps 0 .. K-1 more than once; dpooled dyadic with inf, NaN and -0.0 in its first rows"""
    rng = np.random.default_rng(300 + K)
    shape = (1, 3, K + 5)
    arg = (np.arange(3 * (K + 5)) % K).astype(np.int32).reshape(shape)
    dp = go.dyadic(rng, shape, 4, 8)
    dp.reshape(-1)[:4] = [np.inf, np.nan, -0.0, -np.inf]
    return dp, arg


@pytest.mark.parametrize("K", go.GROUP_MAX_K)
def test_group_max_backward_routes_to_arg_and_zeroes_the_rest(K):
    from usip_amd import ops
    dp, arg = _backward_case(K)
    assert len(np.unique(arg)) == K
    want = go.max_backward(dp, arg, K)
    dz = ops.group_max_backward(_dev(dp), _dev(arg), K)
    assert np.array_equal(_bits(dz), go.bits(want))                         # NaN, inf and -0.0 moved as they are
    off = np.ones(want.shape, bool)
    np.put_along_axis(off, arg.astype(np.int64)[..., None], False, axis=-1)
    assert not _bits(dz)[off].any()                                         # every other slot is +0.0


@pytest.mark.parametrize("K", go.GROUP_MAX_K)
def test_group_max_backward_add_is_one_float32_add_at_arg(K):
    from usip_amd import ops
    dp, arg = _backward_case(K)
    rng = np.random.default_rng(400 + K)
    base = rng.normal(0, 1, dp.shape + (K,)).astype(np.float32)
    want = go.max_backward_add(base, dp, arg)
    dz = _dev(base)
    out = ops.group_max_backward_add_(dz, _dev(dp), _dev(arg))
    assert out.data_ptr() == dz.data_ptr() and _same(dz, want)
    off = np.ones(base.shape, bool)
    np.put_along_axis(off, arg.astype(np.int64)[..., None], False, axis=-1)
    assert np.array_equal(_bits(dz)[off], go.bits(base)[off])               # nobody else's bits move


# ----------------------------------------------------------------------------------------------- autograd wiring
def _lazy(K, relu=True):
    from usip_amd import functional as Fh
    B, C, M = 2, 3, 7
    y, coef, _ = go.act_case(go.act_seed(B, C, M, K), B, C, M, K)
    leaf = _dev(y).view(B, C, M * K).requires_grad_(True)
    rng = np.random.default_rng(500 + K)
    return y, coef, leaf, Fh.LazyAct(leaf, _dev(coef), relu, (B, C, M, K)), go.dyadic(rng, (B, C, M), 4, 8), rng


@pytest.mark.parametrize("K", (16, 12))
def test_autograd_group_max_of_a_tensor(K):
    from usip_amd import functional as Fh
    z = go.pool_case(K, 2 * 3 * 7)[0].reshape(2, 3, 7, K)                  # the special rows among them
    want, arg = go.first_max(z)
    gp = go.dyadic(np.random.default_rng(K), (2, 3, 7), 4, 8)
    zd = _dev(z).requires_grad_(True)
    pooled = Fh.group_max(zd)
    pooled.backward(_dev(gp))
    assert np.array_equal(_bits(pooled), go.bits(want))
    assert np.array_equal(_bits(zd.grad), go.bits(go.max_backward(gp, arg, K)))


@pytest.mark.parametrize("K", (16, 12))
def test_autograd_group_max_of_a_lazy_activation(K):
    """K = 16: _GroupMaxAct, one pass; K = 12: bn_apply, then _GroupMax.  The producer receives the pool's gradient at the
    arg-max of the ACTIVATED values."""
    from usip_amd import functional as Fh
    y, coef, leaf, lazy, gp, _ = _lazy(K)
    want, arg, _ = go.max_act(y, coef, True)
    pooled = Fh.group_max(lazy)
    pooled.backward(_dev(gp))
    assert np.array_equal(_bits(pooled), go.bits(want))
    assert np.array_equal(_bits(leaf.grad).reshape(y.shape), go.bits(go.max_backward(gp, arg, K)))


def test_autograd_group_max_fork_adds_the_pool_gradient_into_the_dense_one():
    from usip_amd import functional as Fh
    K = 16
    y, coef, leaf, lazy, gp, rng = _lazy(K)
    want, arg, _ = go.max_act(y, coef, True)
    dense = go.dyadic(rng, y.shape, 4, 8)
    pooled, passed = Fh.group_max_fork(lazy)
    assert isinstance(passed, Fh.LazyAct) and passed.relu and passed.shape == lazy.shape
    torch.autograd.backward([pooled, passed.y], [_dev(gp), _dev(dense).view(leaf.shape)])
    assert np.array_equal(_bits(pooled), go.bits(want))
    assert np.array_equal(_bits(leaf.grad).reshape(y.shape), go.bits(go.max_backward_add(dense, gp, arg)))
    # pooled alone downstream: the dense routing
    leaf.grad = None
    pooled, passed = Fh.group_max_fork(lazy)
    pooled.backward(_dev(gp))
    assert np.array_equal(_bits(leaf.grad).reshape(y.shape), go.bits(go.max_backward(gp, arg, K)))


# ----------------------------------------------------------------------------------------------- the kept A/B form
# (L, M, nbatch): rows = 3 M; one batch = 4 * 256 / L rows.  batches = ceil(rows / batch) is ODD where nbatch = 2, so the last
# workgroup holds a partly filled batch and one past the end; at nbatch = 8 it holds one full batch, a row, and six past the end
KNOB_CASES = [(16, 87479, 2), (64, 21869, 2), (16, 349547, 8)]


@pytest.mark.parametrize("L,M,nbatch", KNOB_CASES)
def test_walking_several_batches_per_workgroup_gives_the_same_bits(L, M, nbatch):
    """knob r5_forms bit 3: group_max4_kernel with nbatch > 1 against the form the library uses"""
    from usip_amd import _lib, ops
    K, C = 4 * L, 3
    rows, batch = C * M, 4 * 256 // L
    batches = -(-rows // batch)
    nb = 1
    while nb < 8 and batches // (nb * 2) >= 2048:                           # group.hip: group_max4_batches
        nb *= 2
    assert nb == nbatch and rows % batch % 2 == 1 and batches % nb != 0
    g = torch.Generator(device=DEV).manual_seed(L + M)
    n = K // 4
    y = torch.randint(-n, n + 1, (1, C, M, K), generator=g, device=DEV).float() * float(511 // n) / 64.0
    coef = _dev(np.asarray([[1.5, -0.75, 0.5], [-1.0, 0.25, 2.0], [np.nan] * 3, [np.nan] * 3], np.float32))
    want = ops.group_max_act(y, coef, True, want_yarg=True)
    plain = ops.group_max(y)
    _lib.lib().usip_set_tuning(b"r5_forms", 8)
    try:
        got = ops.group_max_act(y, coef, True, want_yarg=True)
        got_plain = ops.group_max(y)
    finally:
        _lib.lib().usip_set_tuning(b"r5_forms", 0)
    for a, b in zip(got + got_plain, want + plain):
        assert torch.equal(a.view(-1).view(torch.int32), b.view(-1).view(torch.int32))
    # and the library's form is right: the pooled value is the largest activated one, found at arg, and yarg is y there
    act = torch.relu(y * coef[0].view(1, C, 1, 1) + coef[1].view(1, C, 1, 1))
    pooled, arg, yarg = want
    assert torch.equal(pooled, act.amax(dim=3))
    assert torch.equal(act.gather(3, arg.long().unsqueeze(3)).squeeze(3), pooled)
    assert torch.equal(y.gather(3, arg.long().unsqueeze(3)).squeeze(3), yarg)
    assert torch.equal(plain[0], y.amax(dim=3))
    if nbatch == 2:                                                         # the FIRST such k (67 MB: cheap enough here)
        for src, (p, a) in ((act, (pooled, arg)), (y, plain)):
            first = ((src == p.unsqueeze(3)).cumsum(dim=3, dtype=torch.int32) == 0).sum(dim=3, dtype=torch.int32)
            assert torch.equal(first, a)


# ----------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize("K", (16, 256))
def test_a_row_with_a_nan_pools_to_nan_at_the_first_nans_k(K):
    """without ReLU: ops.group_max through both kernel families (the view offset by 4 bytes takes group_max_kernel) and
    group_max_act(relu=False); the NaN stands at every k in turn, alone and with a second one"""
    from usip_amd import ops
    z, claims = go.nan_rows(K)
    first, behind, two = go.nan_floors(K)
    assert claims["first"] == first and claims["behind"] >= behind and claims["two"] >= two, claims
    want_arg = np.argmax(np.isnan(z), axis=1).astype(np.int32)
    assert np.array_equal(go.first_max(z)[1], want_arg)
    for v in (_dev(z).view(1, 2, K, K), _off4(z).view(1, 2, K, K)):
        pooled, arg = ops.group_max(v)
        assert torch.isnan(pooled).all(), (K, v.data_ptr() % 16, int((~torch.isnan(pooled)).sum()))
        assert np.array_equal(arg.cpu().numpy().reshape(-1), want_arg), (K, v.data_ptr() % 16)
    coef = np.asarray([[1.5, -0.75], [0.25, -1.0], [np.nan] * 2, [np.nan] * 2], np.float32)
    y = z.reshape(1, 2, K, K)
    want, want_arg, want_yarg = go.max_act(y, coef, False)
    assert np.isnan(want).all() and np.isnan(want_yarg).all()
    pooled, arg, yarg = ops.group_max_act(_dev(y), _dev(coef), False, want_yarg=True)
    assert torch.isnan(pooled).all() and torch.isnan(yarg).all()
    assert np.array_equal(arg.cpu().numpy(), want_arg)


@pytest.mark.parametrize("K", (16, 256))
def test_under_relu_the_pool_agrees_with_what_bn_apply_writes(K):
    """with ReLU a NaN is 0 to every consumer of y (fmaxf in bn_apply and in the GEMM prologue): the pool is the first-index
    max of exactly that tensor"""
    from usip_amd import ops
    z, _ = go.nan_rows(K)
    coef = np.asarray([[1.5, -0.75], [0.25, -1.0], [np.nan] * 2, [np.nan] * 2], np.float32)
    y, cd = _dev(z.reshape(1, 2, K, K)), _dev(coef)
    seen = ops.bn_apply(y.view(1, 2, K * K), cd, True).view(1, 2, K, K).cpu().numpy()
    assert not np.isnan(seen).any() and np.array_equal(go.bits(seen), go.bits(go.act(z.reshape(1, 2, K, K), coef, True)))
    want, want_arg = go.first_max(seen)
    pooled, arg, yarg = ops.group_max_act(y, cd, True, want_yarg=True)
    assert np.array_equal(arg.cpu().numpy(), want_arg) and np.array_equal(_bits(pooled), go.bits(want))
    assert _same(yarg, np.take_along_axis(z.reshape(1, 2, K, K), want_arg[..., None].astype(np.int64), axis=3)[..., 0])
