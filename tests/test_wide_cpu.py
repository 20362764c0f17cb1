"""What the wide-group work (csrc/group_wide.hip, 256 < K <= 1024) rests on, checked without a GPU: the fixture's conditions, the
oracles at K = 448 against torch, the fixtures of tests/wide_form_cases.py, the dispatch predicate and the C interface."""
import ctypes

import numpy as np
import pytest
import torch

import bn_oracle as bo
import group_oracle as go
import wide_form_cases as wc
from conftest import load_golden


def test_fixture_holds_a_truncated_and_a_padded_ball():
    g = load_golden("descriptor_wide_ball.npz")
    K = int(g["cfg_ball_nsamples"])
    members, idx = g["ball_members"], g["idx/ball_idx"].astype(np.int64)
    assert K == 448 and idx.shape == (2, 3, K) and members.shape == (2, 3)
    assert (members >= K).any() and ((members > 0) & (members < K)).any()
    for b in range(2):
        for m in range(3):
            n = int(min(members[b, m], K))
            row = idx[b, m]
            assert np.all(np.diff(row[:n]) > 0), "the first members of the permuted cloud, in order"
            assert np.all(row[n:] == row[np.arange(K - n) % n]), "a padded ball repeats its members from the first on"
            if members[b, m] >= K:
                assert len(np.unique(row)) == K
    # the indices are the C oracle's on the recorded permutation
    from oracle import detector as od
    kp = torch.from_numpy(np.concatenate([g["anc_kp"], g["pos_kp"]]))
    pc = torch.from_numpy(np.concatenate([g["anc_pc"], g["pos_pc"]]))[:, :, g["perm"]]
    dist = od.pairwise_norm(kp, pc)
    assert np.array_equal(od.ball_query_op(dist, float(g["cfg_ball_radius"]), K).numpy(), idx)
    assert np.array_equal((dist <= float(g["cfg_ball_radius"])).sum(2).numpy(), members)
    assert g["idx/pool_arg_0"].dtype == np.int16 and g["idx/pool_arg_0"].max() > 127 and g["idx/pool_arg_1"].max() < K
    for k, v in g.items():
        if k.startswith("grad/"):
            gn = float(g["grad_norm/" + k[5:]])
            assert abs(np.sqrt((v.astype(np.float64) ** 2).sum()) - gn) <= 1e-6 * max(gn, 1e-30), k


def test_pool_oracle_equals_torch_max_at_448():
    K = 448
    z, _ = go.pool_case(K, 461)
    rows = ~np.isnan(z).any(axis=1)
    want, arg = go.first_max(z)
    tv, ti = torch.max(torch.from_numpy(z[rows]), dim=1)
    assert np.array_equal(go.bits(tv.numpy()) & 0x7fffffff != 0, go.bits(want[rows]) & 0x7fffffff != 0)   # (-0.0 == +0.0 in torch)
    assert np.array_equal(tv.numpy(), want[rows])
    # torch.max names A maximum; the oracle names the FIRST: equal where the maximum is attained once
    once = (z[rows] == want[rows][:, None]).sum(1) == 1
    assert once.sum() > 50 and np.array_equal(ti.numpy()[once], arg[rows][once])
    assert np.all(z[np.arange(len(z))[rows], arg[rows]] == want[rows])
    assert all(not (z[r, :arg[r]] == want[r]).any() for r in np.flatnonzero(rows))
    y, coef, _ = go.act_case(go.act_seed(1, 5, 9, K), 1, 5, 9, K)
    for relu in (False, True):
        p, a, ya = go.max_act(y, coef, relu)
        t = torch.from_numpy(y).double() * torch.from_numpy(coef[0]).double().view(1, 5, 1, 1) + \
            torch.from_numpy(coef[1]).double().view(1, 5, 1, 1)
        t = torch.relu(t) if relu else t
        assert np.array_equal(t.max(dim=3)[0].numpy(), p.astype(np.float64))
        assert np.array_equal(np.take_along_axis(y, a[..., None].astype(np.int64), 3)[..., 0], ya)


@pytest.mark.parametrize("relu", [False, True])
def test_bn_oracle_group_sums_equal_double_autograd_at_448(relu):
    nb, C, P, K = 2, 3, 896, 448
    c = bo.build_case(bo.case_seed(nb, C, P, "wide"), nb, C, P)
    r = bo.reduce_f64(c.dz, c.y, c.coef, c.mean, c.invstd, relu, group=K)
    assert r.gsum.shape == (2, nb, C, P // K)
    dy, dgamma, dbeta = bo.dy_autograd_f64(c.y, c.gamma, c.beta, bo.EPS, relu, c.dz)
    scale = np.abs(dy).max((0, 2))
    mine = bo.dy_f64(r)
    # (the oracle takes the fp32 forward coefficients, autograd the exact batch statistics: 1e-5 of each channel's scale)
    assert (np.abs(mine - dy).max((0, 2)) <= 1e-5 * scale).all()
    # sum_k dY = coef4[0] gsum[0] + coef4[2] gsum[1] + K coef4[3]: what bn_group_dy_sum makes of the per-neighbourhood sums
    sdy = r.coef4[0][None, :, None] * r.gsum[0] + r.coef4[2][None, :, None] * r.gsum[1] + K * r.coef4[3][None, :, None]
    want = mine.reshape(nb, C, P // K, K).sum(-1)
    mag = (np.abs(r.coef4[0])[None, :, None] * r.gmag[0] + np.abs(r.coef4[2])[None, :, None] * r.gmag[1]
           + K * np.abs(r.coef4[3])[None, :, None])
    assert (np.abs(sdy - want) <= 1e-12 * mag).all()
    assert (np.abs(r.dgamma - dgamma) <= 1e-5 * r.H2.sum(0)).all() and (np.abs(r.dbeta - dbeta) <= 1e-5 * r.H1.sum(0)).all()


@pytest.mark.parametrize("name", list(wc.WIDE_GEMM_CASES))
def test_wide_gemm_fixture_record(name):
    c, fx = wc.WIDE_GEMM_CASES[name], wc.wide_gemm_fixture(name)
    r = fx["record"]
    want = fx["want"]
    assert np.array_equal(want.astype(np.float64).astype(np.float32), want) and np.count_nonzero(want) > 0
    assert fx["rb_group"] == 448 and fx["rowbias"].shape == (c["nb"], c["M"], c["P"] // 448)
    assert r["rb_straddles_tile"] and r["rb_groups_differ"] and r["tiles_without_b"] == 0 and r["tiles_without_c"] == 0
    assert r["relu_off"] and r["relu_on"] and r["mask_tie"] and r["stats_slots_differ"]
    if c["mode"] == "f32x2":
        assert r["bound_tight"] and r["below_bound"] and r["equals_bound"]
    # 448 = 7 * 64: tiles of 128 and of 256 positions hold two groups (the first one at 384), tiles of 64 never do
    assert any((t // 448) != ((t + 127) // 448) for t in range(0, c["P"], 128)) and 448 % 64 == 0


@pytest.mark.parametrize("name", list(wc.WIDE_LAYER_CASES))
def test_wide_layer_fixture_record(name):
    c, fx = wc.WIDE_LAYER_CASES[name], wc.wide_layer_fixture(name)
    r = fx["record"]
    assert r["pooled"] == 448 and r["below_bound"] and r["tiles_without"] == [0, 0, 0] and r["arg_first"] and r["arg_last"]
    assert r["neighbour_runs_differ"] and r["y_off"] and r["y_on"] and r["x_off"] and r["x_on"]
    assert fx["pool"][2] == 448 and fx["pool"][1].max() == 447 and fx["pool"][1].min() == 0
    if c["opt"].get("gsum"):
        assert fx["red"]["gsum"].shape == (2, 2, 128, 3)


PATHS = {4: "fused", 16: "fused", 64: "fused", 128: "fused", 256: "fused", 12: "fallback", 5: "fallback", 65: "fallback",
         260: "fallback", 264: "fallback", 272: "fallback", 288: "wide", 320: "wide", 448: "wide", 480: "wide", 508: "fallback",
         512: "wide", 768: "wide", 1020: "fallback", 1024: "wide", 1028: "fallback", 1056: "fallback", 2048: "fallback"}


def test_dispatch_predicate():
    """K -> path: the narrow fused forms as they were; the wide kernels for 256 < K <= 1024 with K % 32 == 0 (the GEMM and
    layer-backward forms with a row bias or a pooled group need % 32); everything else on the fallback; WIDE_GROUPS off sends
    every wide K back to the fallback and changes nothing below 256."""
    from usip_amd import functional as Fh
    from usip_amd import ops
    prev = ops.WIDE_GROUPS
    try:
        ops.WIDE_GROUPS = True
        assert {K: Fh._group_path(K) for K in PATHS} == PATHS
        ops.WIDE_GROUPS = False
        assert {K: Fh._group_path(K) for K in PATHS} == {K: ("fallback" if p == "wide" else p) for K, p in PATHS.items()}
    finally:
        ops.WIDE_GROUPS = prev
    assert all(Fh._group_sums_supported(K) == (p == "fused") for K, p in PATHS.items())


def test_the_two_entries_load_through_the_signature_reader():
    from usip_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["usip_group_max_wide_f32"] == ([P, P, I, P, P, P, I, I, I, I, P], I)
    assert _lib.SIGNATURES["usip_bn_backward_reduce_wide_f32"] == _lib.SIGNATURES["usip_bn_backward_reduce_f32"]
    assert _lib.SIGNATURES["usip_group_max_wide_f32"] == _lib.SIGNATURES["usip_group_max_act_f32"]
    lib = _lib.lib()
    assert lib.usip_group_max_wide_f32.argtypes == _lib.SIGNATURES["usip_group_max_wide_f32"][0]
    # refusals that need no device: nothing is launched for them
    assert lib.usip_group_max_wide_f32(None, None, 0, None, None, None, 1, 1, 1, 256, None) != 0
    assert lib.usip_group_max_wide_f32(None, None, 0, None, None, None, 1, 1, 0, 448, None) == 0
    assert lib.usip_bn_backward_reduce_wide_f32(None, None, None, None, None, None, 1, None, None, None, None, None, 448, 1, 1,
                                                448, 0, None) != 0
