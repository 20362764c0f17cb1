"""The fixtures of tests/layer_bwd_oracle.py on the CPU: every case of tests/layer_bwd_cases.py is built and its record asserted
(the builders assert their own exactness claims on the way), the restated walks and plans are pinned to the library's host
entries, and the case table is held against the two dispatchers' own launch lists.  No GPU."""
import os
import re

import numpy as np
import pytest

import layer_bwd_cases as lc
import layer_bwd_oracle as lo

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "usip_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from usip_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ records
@pytest.mark.parametrize("name", list(lc.LAYER_CASES))
def test_layer_fixture_is_exact_and_holds_every_population(name):
    c = lc.LAYER_CASES[name]
    o = c["opt"]
    fx = lc.layer_case_fixture(name)
    r = fx["record"]
    assert fx["blocks"] == c["wgs"]
    assert r["tiles_without"] == [0, 0, 0], r                   # every tile: a W-low, a dY-low and an act(X)-low product
    assert r["below_bound"] and r["zeros"] and all(n > 0 for n in r["neg_zero"]), r
    assert r["y_off"] and r["y_on"] and r["x_off"] and r["x_on"] and r["y_ties"] > 0 and r["x_ties"] > 0, r
    assert r["dx_nonzero"] > 0 and r["dw_nonzero"] > 0
    if o.get("red"):
        assert r["x_tie_with_dx"] > 0 and r["x_off_with_dx"] > 0 and r["workgroup_rows_differ"], r
        assert np.all(fx["red"]["sums"][:, fx["red"]["idle"]] == 0) and np.all(fx["red"]["maxima"][fx["red"]["idle"]] == 0)
    if o.get("pooled"):
        assert r["arg_first"] and r["neighbour_runs_differ"], r
        assert r["arg_ends_on_walk_edges"] == r["walk_edges"], r
        assert r["arg_last"]
    if o.get("ws"):
        assert r["ws_rows_beyond_zero"] and r["wsum_nonzero"] > 0
        assert fx["wsum"].shape == (c["wgs"], 64, 16) and fx["wsum3"].shape == (c["wgs"], 8)


def test_layer_walks_meet_every_edge_the_kernels_have():
    rec = {n: lc.layer_case_fixture(n)["record"] for n in
           ("64x64 one tile", "64x64 second tile in another cloud, wider X", "x2ws three and four tiles, eight rows, wider W",
            "pooled gsum group 128, fewer runs than workgroups", "pooled gsum group 96, two workgroups take two runs",
            "pooled group 24 straddles tiles, three and four")}
    assert rec["64x64 one tile"]["tiles_per_workgroup"] == [1]
    second = rec["64x64 second tile in another cloud, wider X"]
    assert second["tiles_per_workgroup"] == [1, 2] and second["walk_crosses_clouds"]
    assert rec["x2ws three and four tiles, eight rows, wider W"]["tiles_per_workgroup"] == [3, 4]
    idle = rec["pooled gsum group 128, fewer runs than workgroups"]
    assert idle["idle_workgroups"] == 18 and idle["tiles_per_workgroup"] == [0, 4]
    assert rec["pooled gsum group 96, two workgroups take two runs"]["tiles_per_workgroup"] == [3, 6]
    assert rec["pooled group 24 straddles tiles, three and four"]["tiles_per_workgroup"] == [3, 4]
    tiles = {}
    for c in lc.LAYER_CASES.values():
        o = c["opt"]
        _, walk = lo.layer_walk(c["cin"], c["cout"], c["P"], c["nb"], o["pooled"] // 32 if o.get("gsum") else 1)
        tiles.setdefault(c["kernel"], set()).update(len(t) for t in walk)
    for k in (lc.L64, lc.L64R, lc.L64WS, lc.L128, lc.L128R, lc.LPG):
        assert {1, 2, 3, 4} <= tiles[k], (k, tiles[k])          # prologue, steady state and drain of every pipeline
    assert {1, 2, 3} <= tiles[lc.LP] and {0, 1, 2, 3, 4, 6} <= tiles[lc.LPR]


@pytest.mark.parametrize("name", list(lc.NARROW_CASES))
def test_narrow_fixture_is_exact(name):
    c = lc.NARROW_CASES[name]
    fx = lc.narrow_case_fixture(name)
    r = fx["record"]
    assert fx["blocks"] == c["wgs"] and (r["seglen"], r["segs"]) == (c["seglen"], c["segs"])
    assert r["zeros"] and r["y_off"] and r["y_on"] and r["y_ties"] > 0 and all(n > 0 for n in r["neg_zero"]), r
    assert fx["coef4"].shape == (4, c["cout"])
    if c["xpro"]:
        assert r["x_off"] and r["x_on"] and r["x_ties"] > 0
    else:
        assert r["x_negative"] and fx["xcoef"] is None
    if c["red"]:
        assert r["x_tie_with_dx"] > 0 and r["workgroup_rows_differ"], r


def test_narrow_cases_meet_one_and_several_tiles_and_a_short_segment():
    by = {}
    for c in lc.NARROW_CASES.values():
        _, walk = lo.narrow_walk(c["cout"], c["P"], c["nb"])
        by.setdefault(c["kernel"], set()).update(len(t) * 32 for t in walk)
    for k in lc.NARROW_DISPATCH:
        assert {64, 256} <= by[k], (k, by[k])                   # a one-tile segment, a short last one, a full one


# ------------------------------------------------------------------------------------------------ the library's host entries
SHAPES = [(64, 64, 64, 1), (64, 64, 5504, 3), (64, 64, 16448, 3), (64, 128, 16448, 3), (128, 128, 192, 1), (128, 128, 8256, 3),
          (128, 128, 768, 1), (64, 64, 16384, 2), (64, 128, 32768, 16)]


def test_restated_block_counts_are_the_librarys(lib):
    for cin, cout, P, nb in SHAPES:
        want = lo.layer_bwd_blocks(cin, cout, P, nb)
        assert int(lib.usip_mlp_layer_backward_x2h_blocks(cin, cout, P, nb)) == want
        assert int(lib.usip_mlp_layer_backward_x2h_workspace(cin, cout, P, nb)) == want * cout * cin
    for c in lc.LAYER_CASES.values():
        assert int(lib.usip_mlp_layer_backward_x2h_blocks(c["cin"], c["cout"], c["P"], c["nb"])) == c["wgs"]
        assert int(lib.usip_mlp_layer_backward_x2h_supported(c["cin"], c["cout"], c["P"], 1 if c["opt"].get("pooled") else 0)) == 1


def test_restated_narrow_plan_is_the_librarys(lib):
    shapes = [(c["cout"], c["P"], c["nb"]) for c in lc.NARROW_CASES.values()]
    shapes += [(64, 4160, 48), (128, 2112, 64), (64, 320, 768), (128, 320, 1000), (64, 131072, 16), (128, 65536, 1), (64, 64, 1)]
    for cout, P, nb in shapes:
        seglen, segs = lo.narrow_plan(cout, P, nb)
        assert seglen % 64 == 0 and seglen >= 256
        assert int(lib.usip_mlp_narrow_backward_blocks(cout, P, nb)) == nb * segs, (cout, P, nb)
        assert int(lib.usip_mlp_narrow_backward_workspace(cout, P, nb)) == nb * segs * cout * 64
    assert lo.narrow_plan(64, 4160, 48) == (320, 13)            # more than four tiles per segment


def test_supported_shapes(lib):
    sup = lib.usip_mlp_layer_backward_x2h_supported
    assert [int(sup(64, 64, 64, 0)), int(sup(64, 128, 64, 0)), int(sup(128, 128, 64, 1))] == [1, 1, 1]
    for cin, cout, P, pooled in ((64, 64, 32, 0), (64, 64, 96, 0), (64, 64, 0, 0), (128, 128, 64, 0), (64, 64, 64, 1),
                                 (64, 128, 64, 1), (128, 64, 64, 0), (32, 64, 64, 0), (64, 64, 1 << 24, 0), (128, 128, 1 << 23, 1)):
        assert int(sup(cin, cout, P, pooled)) == 0, (cin, cout, P, pooled)
    nsup = lib.usip_mlp_narrow_backward_supported
    assert [int(nsup(64, 64, 64)), int(nsup(64, 128, 320))] == [1, 1]
    assert [int(nsup(64, 64, 32)), int(nsup(128, 128, 64)), int(nsup(64, 96, 64)), int(nsup(64, 64, 0))] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the dispatchers
def _launched(path, kernel, defaults):
    """the instantiations a source file hands to USIP_LAUNCH, spelled as the launch log spells them"""
    text = open(os.path.join(CSRC, path)).read()
    out = []
    for args in re.findall(r"USIP_LAUNCH\(\(?%s<([^>]*)>" % kernel, text):
        a = [s.strip() for s in args.split(",")]
        out.append("%s<%s>" % (kernel, ", ".join(a + defaults[len(a):])))
    return out


def test_every_dispatchable_instantiation_has_a_case():
    layer = _launched("layer_bwd_x2.hip", "layer_bwd_x2_kernel", ["", "", "", "", "", "", "", "false", "false"])
    layer += _launched("layer_bwd_x2.hip", "layer_bwd_x2ws_kernel", [])
    assert sorted(layer) == sorted(lc.LAYER_DISPATCH) and len(set(layer)) == 8
    narrow = _launched("narrow_bwd.hip", "narrow_bwd_kernel", [])
    assert sorted(narrow) == sorted(lc.NARROW_DISPATCH) and len(set(narrow)) == 6
    assert "USIP_LAUNCH(%s," % lc.FINALIZE in open(os.path.join(CSRC, "layer_bwd_x2.hip")).read()
    assert {c["kernel"] for c in lc.LAYER_CASES.values()} == set(lc.LAYER_DISPATCH)
    assert {c["kernel"] for c in lc.NARROW_CASES.values()} == set(lc.NARROW_DISPATCH)
    ws = sorted(c["opt"]["ws"] for c in lc.LAYER_CASES.values() if c["kernel"] == lc.L64WS)
    assert {1, 7, 8} <= set(ws)
    groups = lambda k, gs: sorted({c["opt"]["pooled"] for c in lc.LAYER_CASES.values() if c["kernel"] == k and
                                   bool(c["opt"].get("gsum")) == gs})                                   # noqa: E731
    assert groups(lc.LP, False) == [1, 16, 24, 48] and groups(lc.LPG, False) == [32, 64, 96]
    assert groups(lc.LPR, False) == [32, 64, 96, 128] and groups(lc.LPR, True) == [32, 64, 96, 128]


# ------------------------------------------------------------------------------------------------ the finalise reference
@pytest.mark.parametrize("blocks", lc.FINALIZE_BLOCKS)
def test_wsum_finalize_reference_on_synthetic_sums(blocks):
    for rows in lc.FINALIZE_ROWS:
        wsum, wsum3, coef4, mean = lo.wsum_synthetic(blocks, 64, rows)
        out = lo.wsum_finalize_ref(wsum, wsum3, coef4, mean, rows)
        assert out.shape == (64, rows) and np.count_nonzero(out) > 0
        assert len(np.unique(wsum.reshape(blocks, -1), axis=0)) == blocks
        # the mean term is there: without it some element differs
        no_mu = lo.wsum_finalize_ref(wsum, wsum3, coef4, np.zeros_like(mean), rows)
        assert not np.array_equal(no_mu, out)


def test_producing_layer_fixture_is_exact_in_fp32_as_well():
    """the pair test's fixture: the finalised sums ARE the producing layer's weight gradient, and that product is exact in fp32"""
    fx = lo.layer_fixture(64, 64, 2, 1024, red=True, ws_rows=5, seed=3, w_log2=1)
    coef4, mean, want = lo.producing_layer(fx)
    assert want.shape == (64, 5) and np.count_nonzero(want) > 200 and fx["blocks"] == 64


@pytest.mark.parametrize("kind,name", [("layer", "64x64 red second tile in another cloud"),
                                       ("layer", "pooled red group 96, one and two tiles"),
                                       ("narrow", "narrow 128 xpro red short last segment")])
def test_finalised_bound_covers_the_true_maximum_within_the_documented_factor(kind, name):
    c = (lc.LAYER_CASES if kind == "layer" else lc.NARROW_CASES)[name]
    fx = (lc.layer_case_fixture if kind == "layer" else lc.narrow_case_fixture)(name)
    dg, db, c4, nent = lo.bn_finalize_ref(fx["red"]["sums"], fx["red"]["maxima"], c["nb"] * c["P"], fx["xcoef"])
    true_max = lo.true_dy_maxima(fx, c4)
    assert np.all(c4[4, :nent] >= true_max) and np.all(c4[4, :nent] <= 64 * true_max)
    assert np.count_nonzero(dg) > 0 and np.count_nonzero(db) > 0 and np.count_nonzero(c4[2]) > 0 and np.count_nonzero(c4[3]) > 0
