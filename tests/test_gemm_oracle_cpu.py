"""tests/gemm_oracle.py against independent evaluations, and the claims of every fixture the GPU tests of the shared-MLP
product family use (tests/test_gemm_forms_gpu.py, tests/test_wgrad_forms_gpu.py) -- checked here, on the CPU, before anything
runs on a GPU: the planes reproduce the operands, dropped plane pairs are zero, sums stay below 2^24 units, the true maximum
is within the bound the kernel derives, and every fixture holds the value classes and edges it exists for."""
import math

import numpy as np
import pytest
import torch

import gemm_cases as gc
import gemm_oracle as go

SMALL = [n for n, c in gc.GEMM_CASES.items() if c["nb"] * c["P"] * max(c["M"], c["K"]) <= 1 << 22]


def test_pow2_scale_and_weight_scale():
    for bound, top in [(1.0, 15), (1.5, 15), (2.0, 15), (3e-7, 15), (7e4, 15), (1.0, 14), (0.999, 14)]:
        s = float(go.pow2_scale(bound, top))
        assert 2.0 ** (top - 1) <= bound * s < 2.0 ** top and math.frexp(s)[0] == 0.5
    assert float(go.pow2_scale(0.0, 14)) == 2.0 ** 60                       # an all-zero operand
    assert float(go.pow2_scale(np.inf, 15)) == 1.0
    assert float(go.pow2_scale(1e-30, 15)) == 2.0 ** 60 and float(go.pow2_scale(1e30, 15)) == 2.0 ** -60
    A = np.array([[0.0, -3.0], [0.5, 1.0]], np.float32)
    assert 2.0 ** 13 <= 3.0 * float(go.weight_scale(A)) < 2.0 ** 14
    assert float(go.weight_scale(np.zeros((2, 2), np.float32))) == 2.0 ** 60


def test_split_models_match_torch_casts():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 300.0,
                        np.array([0.0, -0.0, 1.0, 257.0, 259.0, 2049.0, 8197.0, 131329.0, 2.0 ** 14, 65504.0 / 4], np.float32)])
    t = torch.from_numpy(x)
    x16, t16 = x[np.abs(x) < 65504.0], t[t.abs() < 65504.0]
    hi, lo = go.split2h(x16)
    thi = t16.to(torch.float16)
    tlo = (t16 - thi.float()).to(torch.float16)
    assert np.array_equal(hi.view(np.uint16), thi.numpy().view(np.uint16))
    assert np.array_equal(lo.view(np.uint16), tlo.numpy().view(np.uint16))
    h, m, l = go.split3(x)
    th = t.to(torch.bfloat16).float()
    tm = (t - th).to(torch.bfloat16).float()
    tl = (t - th - tm).to(torch.bfloat16).float()
    for mine, theirs in ((h, th), (m, tm), (l, tl)):
        assert np.array_equal(go.bits(mine), go.bits(theirs.numpy()))
    assert float(np.abs(x - h - m - l).max()) <= float(np.abs(x).max()) * 2.0 ** -24


def test_image_layout_roundtrip():
    """image_ref places element (row, k) of stage (mt, ks), plane s at 16-bit index ((mt nks + ks) npl + s) bm 16 +
    lds_off(row, k / 8) / 2 + k % 8 -- restated here element by element."""
    rng = np.random.default_rng(2)
    A = rng.integers(-300, 300, (130, 17)).astype(np.float32)
    for bm, form in ((128, "x3"), (256, "x2h")):
        img, scale = go.image_ref(A, bm, form)
        npl, nks = go.NPLANES[form], 2
        planes = go.split3(A) if form == "x3" else [p.astype(np.float32) for p in go.split2h(A * scale)]
        for (m, k) in [(0, 0), (7, 8), (8, 8), (8, 0), (129, 16), (127, 15), (15, 9)]:
            mt, row, ks, kk = m // bm, m % bm, k // 16, k % 16
            for s in range(npl):
                idx = ((mt * nks + ks) * npl + s) * bm * 16 + go.lds_off(row, kk // 8) // 2 + kk % 8
                got = img[idx]
                want = (go.bits(planes[s][m, k]).reshape(-1)[0] >> 16) if form == "x3" else np.float16(planes[s][m, k]).view(np.uint16)
                assert int(got) == int(want), (form, m, k, s)
        assert img.size * 2 == go.image_bytes(130, 17, bm, npl)
        assert np.count_nonzero(img) <= npl * np.count_nonzero(A)         # everything beyond M x K is zero


@pytest.mark.parametrize("name", SMALL)
def test_fixture_product_matches_torch_float64(name):
    """the oracle's prologue and product against torch.float64 on the same operands"""
    c, fx = gc.GEMM_CASES[name], gc.case_fixture(name)
    pro, K = c["pro"], c["K"]
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).double()          # noqa: E731
    cf = t(fx["coef"])
    if pro == 0:
        V = t(fx["X"])
    elif pro == 1:
        V = torch.relu(t(fx["X"]) * cf[0].view(1, K, 1) + cf[1].view(1, K, 1))
    else:
        y = t(fx["X2"])
        if pro == 3:
            dp, arg, g = fx["pool"]
            dz = torch.zeros_like(y).view(c["nb"], K, -1, g)
            dz.scatter_(3, torch.from_numpy(arg).long().unsqueeze(-1), t(dp).unsqueeze(-1))
            dz = dz.view_as(y)
        else:
            dz = t(fx["X"])
        on = (y * cf[0].view(1, K, 1) + cf[1].view(1, K, 1)) > 0
        V = cf[0].view(1, K, 1) * torch.where(on, dz, torch.zeros_like(dz)) + (cf[2].view(1, K, 1) * y + cf[3].view(1, K, 1))
    Y = torch.einsum("mk,bkp->bmp", t(fx["A"]), V)
    if fx["bias"] is not None:
        Y = Y + t(fx["bias"]).view(1, -1, 1)
    if fx["rowbias"] is not None:
        Y = Y + t(fx["rowbias"]).repeat_interleave(fx["rb_group"], dim=2)
    if c["opt"].get("fork"):
        dp, arg, g = fx["fork"]
        Yv = Y.view(c["nb"], c["M"], -1, g)
        Yv.scatter_add_(3, torch.from_numpy(arg).long().unsqueeze(-1), t(dp).unsqueeze(-1))
    assert torch.equal(Y, t(fx["want"]))
    if fx["stats"] is not None and not c["opt"].get("walk"):
        tile = 256 if c["M"] <= 64 else 128
        for b in range(c["nb"]):
            for i in range(0, c["P"], tile):
                slot = b * ((c["P"] + tile - 1) // tile) + i // tile
                seg = Y[b, :, i:i + tile]
                assert torch.equal(seg.sum(1), t(fx["stats"][0, :, slot])) and torch.equal((seg * seg).sum(1), t(fx["stats"][1, :, slot]))


@pytest.mark.parametrize("name", list(gc.GEMM_CASES))
def test_fixture_record(name):
    """what each fixture must hold (the builder has already asserted exactness, planes, dropped pairs and the bound)"""
    c, fx = gc.GEMM_CASES[name], gc.case_fixture(name)
    r, o = fx["record"], c["opt"]
    want32 = fx["want"]
    assert np.array_equal(want32.astype(np.float64).astype(np.float32), want32) and np.all(np.isfinite(want32))
    assert np.count_nonzero(want32) > 0
    if c["form"] != "a" and c["K"] >= 16:
        assert r["class_b"] and r["class_c"], "both low-plane populations"
        last = (c["K"] - 1) // 16
        in_last = [any(k // 16 == last for k in r[key]) for key in ("b_channels", "c_channels")]
        assert all(in_last) if c["K"] % 16 == 0 or c["K"] % 16 >= 4 else any(in_last), "low planes in the last 16-k stage"
        assert any(k // 16 == 0 for k in r["b_channels"]) and any(k // 16 == 0 for k in r["c_channels"])
        assert r["tiles_without_b"] == 0 and r["tiles_without_c"] == 0, "every tile of 64 positions meets both populations"
    if c["form"] == "a":
        assert not r["class_b"] and not r["class_c"]
    if c["K"] >= 16:
        assert r["zeros"] and (r["neg"] or c["pro"] == 1)
        if c["pro"] >= 1:
            assert r["relu_off"] and r["relu_on"] and r["mask_tie"]
    if c["form"] == "x2h" and c["mode"] == "f32x2":
        assert r["bound_tight"] and r["below_bound"]
        assert r["a_scale"] * float(np.abs(fx["A"]).max()) >= 2.0 ** 13
        assert r["equals_bound"], "one element equal to the bound the kernel derives"
    if o.get("rb"):
        # a group can straddle a tile edge only where it does not divide the tile; neighbouring groups never hold the same values
        assert r["rb_straddles_tile"] == (c["P"] > 128 and 128 % o["rb"] != 0)
        assert r["rb_groups_differ"]
    if o.get("fork"):
        assert r["fork_arg_first"] and r["fork_arg_last"]
    if c["pro"] == 3:
        assert r["arg_first"] and r["arg_last"]
    if "red" in o:
        assert r["red_mask_tie"] and r["red_mask_off"] and fx["red"]["sums"].any() and fx["red"]["maxima"].all()
    if fx["stats"] is not None and r["stats_slots"] > 1:
        assert r["stats_slots_differ"]


def test_row_bias_group_straddles_a_tile():
    fx = gc.case_fixture("f32 32-row pro1 ragged")                        # rb_group 3: 255 | 256 | 257 share a group
    assert fx["record"]["rb_straddles_tile"]
    rb = fx["rowbias"]
    assert rb.shape == (3, 31, 111) and np.any(rb[:, :, 256 // 3] != 0)


def test_x2r_walk():
    G, walk = go.x2r_walk(1, 33288)
    assert G == 512 and sum(len(w) for w in walk) == 521 and walk[0] == [(0, 0), (0, 512)] and walk[8] == [(0, 8), (0, 520)]
    assert walk[9] == [(0, 9)]
    G, walk = go.x2r_walk(2, 200)
    assert G == 8 and walk[5] == [(1, 1)]


@pytest.mark.parametrize("name", list(gc.WGRAD_CASES))
def test_wgrad_fixture(name):
    """the weight-gradient fixtures: the builder asserts planes, dropped pairs, the bounds and the 2^24 condition; here the
    product against torch.float64, the value classes and the segment plan each case exists for"""
    c, fx = gc.WGRAD_CASES[name], gc.wgrad_case_fixture(name)
    r = fx["record"]
    t = lambda a: torch.from_numpy(np.asarray(a)).double()                 # noqa: E731
    M, N, pro = c["M"], c["N"], c["pro"]
    if pro == 0:
        V = t(fx["G"])
    else:
        cf, y = t(fx["coef4"]), t(fx["G2"])
        if pro == 3:
            dp, arg, g = fx["pool"]
            dz = torch.zeros_like(y).view(c["nb"], M, -1, g)
            dz.scatter_(3, torch.from_numpy(arg).long().unsqueeze(-1), t(dp).unsqueeze(-1))
            dz = dz.view_as(y)
        else:
            dz = t(fx["G"])
        on = (y * cf[0].view(1, M, 1) + cf[1].view(1, M, 1)) > 0
        V = cf[0].view(1, M, 1) * torch.where(on, dz, torch.zeros_like(dz)) + (cf[2].view(1, M, 1) * y + cf[3].view(1, M, 1))
    X = t(fx["X"])
    if fx["xcoef"] is not None:
        xc = t(fx["xcoef"])
        X = torch.relu(X * xc[0].view(1, N, 1) + xc[1].view(1, N, 1))
    assert torch.equal(torch.einsum("bmp,bnp->mn", V, X), t(fx["want"]))
    assert r["nonzero_out"] > 0
    if c["form"] != "a":
        assert r["class_g_low"] and r["class_x_low"]
    if pro >= 2:
        assert r["mask_tie"]
    if "short last segment" in name or name in ("x3 256 tiles", "x2l pro2"):
        assert c["segs"] > 2 and 0 < c["P"] - (c["segs"] - 1) * c["seglen"] < 32 and (c["P"] // 16) % 2 == 1
    if name == "f32 one slice":
        assert c["segs"] == 1 and c["nb"] == 1
    if name == "f32 two slices coloff":
        assert c["segs"] == 2


def test_every_recorded_route_has_an_exact_case():
    """every GEMM instantiation tests/golden/gemm_routes_parent.json records is the target of at least one exact case"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes_parent.json")) as f:
        rows = json.load(f)["rows"]
    targets = {c["kernel"] for c in gc.GEMM_CASES.values()}
    for name, row in rows.items():
        gemm = row["launches"][-1][0]                           # (the weight split first, the GEMM last)
        assert any("::" + t + "(" in gemm for t in targets), (name, gemm)
