"""The pooling kernel for neighbourhoods wider than 256 samples (csrc/group_wide.hip: group_max_wide_kernel<NP, NANS>) against
tests/group_oracle.py, bit for bit: dyadic inputs, nothing rounds.

A row belongs to one wave; lane l owns the float4s l + 64 j, j < NP = ceil(K / 256).  So element k sits on lane (k // 4) % 64
in pass k // 256, and two equal maxima can meet inside a lane (k and k + 256), across the lanes of one pass, or crosswise: k = 100
is lane 25 of pass 0, k = 260 is lane 1 of pass 1 -- the lower k on the higher lane.  K = 260 leaves one lane in the second pass,
K = 1020 idles the last lane of the last pass.  NP = 2 gives a wave two rows, NP = 3, 4 one: the ragged row counts (8 n + 5)
leave a wave with one of its two rows, a wave with none, and a workgroup partly filled."""
import ctypes

import numpy as np
import pytest
import torch

import group_oracle as go
from gemm_gpu_helpers import DEV, _dev, _logged

pytestmark = pytest.mark.gpu
WIDE_K = (260, 320, 448, 508, 512, 768, 1020, 1024)


def _off4(a):
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
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


def ragged(K):
    """rows = 8 n + 5 >= K + the special rows: every k is a first maximum once, and the last workgroup is partly filled"""
    return 8 * (-(-(K + go.SPECIAL_ROWS) // 8)) + 5


def wide_tie_claims(z):
    """rows of z [R,K] whose maximum is attained twice or more on ONE lane in two passes / on two lanes (oracle only)"""
    cross_pass = cross_lane = 0
    for r in range(z.shape[0]):
        t = np.flatnonzero(z[r] == z[r].max())
        lanes, passes = (t // 4) % 64, t // 256
        cross_lane += len(np.unique(lanes)) > 1
        cross_pass += any(len(np.unique(passes[lanes == l])) > 1 for l in np.unique(lanes))
    return int(cross_pass), int(cross_lane)


@pytest.mark.parametrize("K", WIDE_K)
def test_group_max_wide_equals_the_first_index_max(K):
    from usip_amd import _lib, ops
    for R in (1, 3, ragged(K)):
        z, _ = go.pool_case(K, R)
        if R > 3:
            z = z.copy()
            z[K + 1, [1, 257]] = 8.0                      # above every value: lane 0 holds the maximum in passes 0 and 1
            cross_pass, cross_lane = wide_tie_claims(z[:R - go.SPECIAL_ROWS])
            assert cross_pass >= 1 and cross_lane >= 1, (K, cross_pass, cross_lane)
            assert len(np.unique(np.argmax(z[:K], axis=1))) == K                      # the first maximum visits every k
        want, want_arg = go.first_max(z)
        (pooled, arg), got = _logged(_lib.lib(), lambda: ops.group_max_wide(_dev(z).view(1, 1, R, K)))
        assert np.array_equal(arg.cpu().numpy().reshape(-1), want_arg), (K, R)
        assert np.array_equal(_bits(pooled).reshape(-1), go.bits(want)), (K, R)
        NP = -(-K // 256)
        per = 8 if NP == 2 else 4
        assert len(got) == 1 and "::group_max_wide_kernel<%d, true>(" % NP in got[0][0] and got[0][1] == -(-R // per), got


@pytest.mark.parametrize("K", WIDE_K)
def test_group_max_wide_ranks_a_nan_above_everything(K):
    from usip_amd import ops
    z, claims = go.nan_rows(K)
    first, behind, two = go.nan_floors(K)
    assert claims["first"] == first and claims["behind"] >= behind and claims["two"] >= two, claims
    first = np.argmax(np.isnan(z), axis=1).astype(np.int32)
    pooled, arg = ops.group_max_wide(_dev(z).view(2, 1, K, K))
    assert torch.isnan(pooled).all()
    assert np.array_equal(arg.cpu().numpy().reshape(-1), first)
    # through the activation without ReLU the NaN of fma(y, 1, 0) wins the same way; with ReLU fmaxf(NaN, 0) = 0 replaced it
    coef = _dev(np.asarray([[1.0], [0.0]], np.float32))
    pooled, arg, yarg = ops.group_max_wide(_dev(z).view(2 * K, 1, 1, K), coef, False, want_yarg=True)
    assert torch.isnan(pooled).all() and torch.isnan(yarg).all()
    assert np.array_equal(arg.cpu().numpy().reshape(-1), first)
    want, want_arg, want_yarg = go.max_act(z.reshape(2 * K, 1, 1, K), np.asarray([[1.0], [0.0]], np.float32), True)
    pooled, arg, yarg = ops.group_max_wide(_dev(z).view(2 * K, 1, 1, K), coef, True, want_yarg=True)
    assert np.array_equal(arg.cpu().numpy(), want_arg) and np.array_equal(_bits(pooled), go.bits(want))
    assert _same(yarg, want_yarg)


ACT_SHAPES = ((1, 1, 1), (1, 3, 1), (1, 5, 9))                 # (B, C, M): 1, 3 and 45 = 8 n + 5 rows


@pytest.mark.parametrize("K", WIDE_K)
def test_group_max_wide_equals_the_activated_first_index_max(K):
    from usip_amd import _lib, ops
    for B, C, M in ACT_SHAPES:
        y, coef, claims = go.act_case(go.act_seed(B, C, M, K), B, C, M, K)
        if M > 1:
            assert claims["tied"] >= 10 and claims["moved"] >= 10 and (claims["negative"], claims["zero"]) == (1, 1) \
                and claims["nonpos"] >= 1, claims                                  # SCALES: -0.75, 0, 0.5 (y/2 - 4 <= 0), 1, 1.5
        assert np.isnan(coef[2:]).all()
        yd, cd = _dev(y), _dev(coef)
        for relu in (False, True):
            want, want_arg, want_yarg = go.max_act(y, coef, relu)
            (pooled, arg, yarg), got = _logged(_lib.lib(), lambda: ops.group_max_wide(yd, cd, relu, want_yarg=True))
            pooled2, arg2 = ops.group_max_wide(yd, cd, relu)
            for p, a in ((pooled, arg), (pooled2, arg2)):
                assert np.array_equal(a.cpu().numpy(), want_arg), (K, (B, C, M), relu)
                assert np.array_equal(_bits(p), go.bits(want)), (K, (B, C, M), relu)
            assert np.array_equal(_bits(yarg), go.bits(want_yarg)), (K, (B, C, M), relu)
            assert "::group_max_wide_kernel<%d, %s>(" % (-(-K // 256), "false" if relu else "true") in got[0][0], got


NAN, INF = float("nan"), float("inf")
# {k: value} among -1.0 everywhere else -> the expected arg, as a literal.  K - 1 is written as -1.
PLACED = [
    ({5: 3.0, 261: 3.0}, 5),                                   # one lane (1), passes 0 and 1
    ({8: 3.0, 200: 3.0}, 8),                                   # two lanes of pass 0
    ({300: 3.0, 280: 3.0}, 280),                               # two lanes of pass 1
    ({100: 3.0, 260: 3.0}, 100),                               # crossing: the lower k on the higher lane
    ({260: 3.0, 100: 2.5}, 260),
    ({100: 0.0, 260: -0.0}, 100),                              # +0.0 before -0.0: they tie, the first wins with ITS bits
    ({100: -0.0, 260: 0.0}, 100),
    ({5: -0.0, 261: 0.0}, 5),
    ({261: 0.0, 8: -0.0, 5: -2.0}, 8),
    ({5: NAN}, 5), ({261: NAN}, 261), ({100: NAN}, 100), ({260: NAN}, 260),
    ({5: NAN, 261: NAN}, 5), ({8: NAN, 200: NAN}, 8), ({300: NAN, 280: NAN}, 280), ({100: NAN, 260: NAN}, 100),
    ({260: NAN, 100: 3.0}, 260), ({261: NAN, 5: INF}, 261),
    ({-1: NAN, 0: INF}, -1),                                   # a NaN in the last pass against +inf in the first
    ({-1: NAN, 3: INF, 7: NAN}, 7),
]


@pytest.mark.parametrize("K", (320, 448, 1020, 1024))
def test_placed_ties_and_nans_pool_to_the_first_k(K):
    from usip_amd import ops
    z = np.full((len(PLACED), K), -1.0, np.float32)
    lit = np.empty(len(PLACED), np.int32)
    for r, (put, k) in enumerate(PLACED):
        for kk, v in put.items():
            z[r, kk % K] = v
        lit[r] = k % K
    want, want_arg = go.first_max(z)
    assert np.array_equal(want_arg, lit)                                           # the literals are the oracle's
    ident = _dev(np.asarray([[1.0], [-0.0]], np.float32))                         # fma(z, 1, -0.0) has the bits of z
    for coef in (None, ident):
        pooled, arg, yarg = ops.group_max_wide(_dev(z).view(1, 1, len(PLACED), K), coef, False, want_yarg=True) \
            if coef is not None else ops.group_max_wide(_dev(z).view(1, 1, len(PLACED), K)) + (None,)
        assert arg.cpu().numpy().reshape(-1).tolist() == lit.tolist()
        assert _same(pooled.view(-1), want)
        assert yarg is None or _same(yarg.view(-1), want)


def test_placed_ties_at_260_where_the_second_pass_holds_one_lane():
    from usip_amd import ops
    K = 260
    placed = [({2: 3.0, 258: 3.0}, 2), ({258: 3.0}, 258), ({259: 3.0, 255: 3.0}, 255), ({257: NAN, 1: NAN}, 1),
              ({259: NAN, 0: INF}, 259), ({256: 0.0, 3: -0.0}, 3), ({256: -0.0, 252: -2.0}, 256)]
    z = np.full((len(placed), K), -1.0, np.float32)
    for r, (put, _) in enumerate(placed):
        for kk, v in put.items():
            z[r, kk] = v
    want, want_arg = go.first_max(z)
    assert want_arg.tolist() == [k for _, k in placed]
    pooled, arg = ops.group_max_wide(_dev(z).view(1, len(placed), 1, K))
    assert arg.cpu().numpy().reshape(-1).tolist() == [k for _, k in placed] and _same(pooled.view(-1), want)


def test_group_max_wide_refuses_what_it_has_no_kernel_for():
    from usip_amd import _lib, ops
    coef = _dev(np.asarray([[1.0, 0.5], [0.0, 0.25]], np.float32))
    for K in (256, 258, 1028):
        for c in (None, coef):
            with pytest.raises(RuntimeError):
                ops.group_max_wide(torch.zeros(1, 2, 3, K, device=DEV), c, True)
    with pytest.raises(RuntimeError):
        ops.group_max_wide(_off4(np.zeros((1, 2, 3, 448), np.float32)), coef, True)
    y = torch.zeros(1, 2, 3, 448, device=DEV)
    pooled = torch.empty(1, 2, 3, device=DEV)
    arg = torch.empty(1, 2, 3, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                    # noqa: E731
    fn = _lib.lib().usip_group_max_wide_f32
    for args in ((None, p(pooled), p(arg)), (p(y), None, p(arg)), (p(y), p(pooled), None)):
        assert fn(args[0], p(coef), 1, args[1], args[2], None, 1, 2, 3, 448, None) != 0
    assert fn(None, None, 0, None, None, None, 1, 2, 0, 448, None) == 0           # zero rows: nothing to do
    torch.cuda.synchronize()
    pooled, arg = ops.group_max_wide(y, coef, True)                                # and takes the aligned one
    assert pooled.cpu().tolist() == [[[0.0] * 3, [0.25] * 3]] and not arg.any()


def test_the_narrow_entries_still_refuse_a_wide_group():
    from usip_amd import ops
    coef = _dev(np.asarray([[1.0, 0.5], [0.0, 0.25]], np.float32))
    with pytest.raises(RuntimeError):
        ops.group_max_act(torch.zeros(1, 2, 3, 512, device=DEV), coef, True)
