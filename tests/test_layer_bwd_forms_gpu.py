"""Every form of the fused layer backward, bit for bit (csrc/layer_bwd_x2.hip: layer_bwd_x2_kernel in seven instantiations,
layer_bwd_x2ws_kernel, wsum_finalize_kernel; csrc/narrow_bwd.hip: narrow_bwd_kernel in six).

Operands from tests/layer_bwd_oracle.py: ONE set per launch for which both products and every side sum are exact -- dY, act(X)
and W reproduced by their two fp16 planes under the scales the kernel derives, per contraction index of either product at most
one low plane, sum |products| below 2^24 units for every dX, every dW over all positions and every per-workgroup partial -- so
the tile walk, the wave roles and the order of the partial sums cannot change a bit and every output must EQUAL the float32 of
the fp64 result, laid out by the restated walk.  No tolerance appears in this file.  Each case asserts from the launch log
which instantiation ran, with the workgroup count of the restated block plan."""
import ctypes

import numpy as np
import pytest
import torch

import layer_bwd_cases as lc
import layer_bwd_oracle as lo
from gemm_gpu_helpers import DEV, _Switches, _dev, _logged, _ran

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _eq(got, want, what):
    want = _dev(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), "%s: %d of %d differ, first at %s" % (
        what, int(bad.sum()), want.numel(), tuple(int(i) for i in bad.nonzero()[0]))


class _Layer:
    """device operands of one layer fixture and the two ways to launch them"""

    def __init__(self, c, fx):
        from usip_amd import ops
        self.c, self.fx, o = c, fx, c["opt"]
        self.cin, self.cout, self.nb, self.P = c["cin"], c["cout"], c["nb"], c["P"]
        self.dz, self.y, self.coef4 = _dev(fx["dZ"]), _dev(fx["Y"]), _dev(fx["coef4"])
        self.x, self.xcoef, self.w = _dev(fx["X"]), _dev(fx["xcoef"]), _dev(fx["Wst"])
        self.pool = None if fx["pool"] is None else (_dev(fx["pool"][0]), _dev(fx["pool"][1]), fx["pool"][2])
        self.wsrc = _dev(fx.get("wsrc"))
        self.red, self.gsum, self.wcol = bool(o.get("red")), bool(o.get("gsum")), fx["wcol"]
        ops.declare_samples(self.xcoef, self.nb * self.P)
        self.dw = _nan(*self.w.shape)

    def through_ops(self):
        from usip_amd import ops
        assert ops.layer_backward_x2_supported(self.cin, self.cout, self.P, (self.dz, self.y, self.x), self.coef4, self.xcoef,
                                               pooled=self.pool is not None)
        out = ops.mlp_layer_backward_x2(self.dz, self.y, self.coef4, self.x, self.xcoef, self.w, wcol=self.wcol, dw_out=self.dw,
                                        Cin=self.cin, want_red=self.red, pool=self.pool, want_gsum=self.gsum, wsrc=self.wsrc)
        dx, red = out[0], (out[2] if self.red else None)
        return dict(dx=dx, sums=red.sums if red else None, maxima=red.maxima if red else None, gsum=red.gsum if red else None,
                    wsum=red.wsum[0] if red and red.wsum else None, wsum3=red.wsum[1] if red and red.wsum else None, red=red)

    def through_c(self, dx_rows, lib):
        """the C entry with every output pre-filled with NaN, dX as rows [0, cin) of a [nb, dx_rows, P] tensor"""
        from usip_amd import ops
        cin, cout, nb, P = self.cin, self.cout, self.nb, self.P
        blocks = int(lib.usip_mlp_layer_backward_x2h_blocks(cin, cout, P, nb))
        dxw = _nan(nb, dx_rows, P)
        ws = _nan(int(lib.usip_mlp_layer_backward_x2h_workspace(cin, cout, P, nb)))
        red = _nan(2 * blocks * cin + blocks) if self.red else None
        planes = ops.weight_planes(self.w, self.wcol, cin, cout, 2, P, nb)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.usip_mlp_layer_backward_x2h_f32(_p(self.dz), _p(self.y), _p(self.coef4), None, None, 0, _p(self.x),
                                                 int(self.x.shape[1]), _p(self.xcoef), _p(planes), _p(dxw), dx_rows, _p(ws),
                                                 _p(self.dw, 4 * self.wcol), int(self.dw.shape[1]), _p(red), None, cin, cout, P,
                                                 nb, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert _all_nan(dxw[:, cin:]), "rows of the wider dX beyond the layer's were written"
        r = ops.RedSums(red, cin) if red is not None else None
        return dict(dx=dxw[:, :cin], sums=r.sums if r else None, maxima=r.maxima if r else None, gsum=None, wsum=None,
                    wsum3=None, red=r)


def _check_layer(L, got):
    fx, wcol, cin = L.fx, L.wcol, L.cin
    _eq(got["dx"], fx["dX"], "dX")
    _eq(L.dw[:, wcol:wcol + cin], fx["dW"], "dW")
    assert _all_nan(L.dw[:, :wcol]) and _all_nan(L.dw[:, wcol + cin:]), "columns of dW outside the operand were written"
    if L.red:
        _eq(got["sums"], fx["red"]["sums"], "red.sums")
        _eq(got["maxima"], fx["red"]["maxima"], "red.maxima")
    if L.gsum:
        _eq(got["gsum"], fx["red"]["gsum"], "gsum")
    if L.wsrc is not None:
        _eq(got["wsum"], fx["wsum"], "wsum")
        _eq(got["wsum3"], fx["wsum3"], "wsum3")


@pytest.mark.parametrize("name", list(lc.LAYER_CASES))
def test_layer_backward_form_equals_the_exact_results(name):
    from usip_amd import _lib
    lib = _lib.lib()
    c = lc.LAYER_CASES[name]
    fx = lc.layer_case_fixture(name)
    with _Switches("f32x2"):
        L = _Layer(c, fx)
        call = (lambda: L.through_c(c["opt"]["c_entry"], lib)) if c["opt"].get("c_entry") else L.through_ops
        got, log = _logged(lib, call)
        torch.cuda.synchronize()
    _ran(log, c["kernel"], c["wgs"])
    assert sum(1 for n, _ in log if "layer_bwd_x2" in n) == 1, log
    _check_layer(L, got)


class _Narrow:
    def __init__(self, c, fx):
        self.c, self.fx = c, fx
        self.dz, self.y, self.coef4 = _dev(fx["dZ"]), _dev(fx["Y"]), _dev(fx["coef4"])
        self.x, self.xcoef, self.w = _dev(fx["X"]), _dev(fx["xcoef"]), _dev(fx["Wst"])
        self.dw = _nan(*self.w.shape)

    def run(self):
        from usip_amd import ops
        c = self.c
        assert ops.narrow_backward_supported(64, c["cout"], c["P"], (self.dz, self.y, self.x))
        return ops.mlp_narrow_backward(self.dz, self.y, self.coef4, self.x, self.xcoef, self.w, wcol=self.fx["wcol"],
                                       dw_out=self.dw, Cin=64, want_red=c["red"])


@pytest.mark.parametrize("name", list(lc.NARROW_CASES))
def test_narrow_backward_form_equals_the_exact_results(name):
    from usip_amd import _lib
    lib = _lib.lib()
    c = lc.NARROW_CASES[name]
    fx = lc.narrow_case_fixture(name)
    with _Switches("f32"):
        N = _Narrow(c, fx)
        out, log = _logged(lib, N.run)
        torch.cuda.synchronize()
    _ran(log, c["kernel"], c["wgs"])
    wcol = fx["wcol"]
    _eq(out[0], fx["dX"], "dX")
    _eq(N.dw[:, wcol:wcol + 64], fx["dW"], "dW")
    assert _all_nan(N.dw[:, :wcol]) and _all_nan(N.dw[:, wcol + 64:])
    if c["red"]:
        _eq(out[2].sums, fx["red"]["sums"], "red.sums")
        _eq(out[2].maxima, fx["red"]["maxima"], "red.maxima")


# ------------------------------------------------------------------------------------------------ the BatchNorm finalisation
FINALIZE_FROM = [("layer", "64x64 red second tile in another cloud"), ("layer", "pooled red group 96, one and two tiles"),
                 ("layer", "64x128 red one tile, wider X"), ("narrow", "narrow 128 xpro red short last segment")]


@pytest.mark.parametrize("kind,name", FINALIZE_FROM)
def test_bn_backward_from_the_exact_partials(kind, name):
    """ops.bn_backward_from_partials on the fixture's own exact partials: dgamma, dbeta and rows 0-3 of coef4 equal the reference
    (the sums in float64, rounded once; the coefficients one float32 operation after the other), row 4 equals the written bound,
    covers the true maximum of |dY| of the producing layer and stays within the documented factor 64 of it."""
    from usip_amd import ops
    c = (lc.LAYER_CASES if kind == "layer" else lc.NARROW_CASES)[name]
    fx = (lc.layer_case_fixture if kind == "layer" else lc.narrow_case_fixture)(name)
    cin = fx["xcoef"].shape[1]
    count = c["nb"] * c["P"]
    dg, db, c4, nent = lo.bn_finalize_ref(fx["red"]["sums"], fx["red"]["maxima"], count, fx["xcoef"])
    true_max = lo.true_dy_maxima(fx, c4)
    flat = _dev(np.concatenate([fx["red"]["sums"].reshape(-1), fx["red"]["maxima"].reshape(-1)]))
    xcoef = _dev(fx["xcoef"])
    got_dg, got_db, got_c4 = ops.bn_backward_from_partials(ops.RedSums(flat, cin), count, xcoef, xcoef[2].contiguous(),
                                                           xcoef[3].contiguous())
    torch.cuda.synchronize()
    assert got_c4.shape == (5, cin)
    _eq(got_dg, dg, "dgamma")
    _eq(got_db, db, "dbeta")
    _eq(got_c4[:4], c4[:4], "coef4[:4]")
    _eq(got_c4[4, :nent], c4[4, :nent], "coef4[4]")
    bound = got_c4[4, :nent].double().cpu().numpy()
    assert np.all(bound >= true_max) and np.all(bound <= 64.0 * true_max), (bound, true_max)


# ------------------------------------------------------------------------------------------------ wsum_finalize
def _finalize(lib, wsum, wsum3, coef4, mean, rows, lddw):
    from usip_amd import ops
    dW = _nan(wsum.shape[1], lddw)
    pack = (_dev(wsum), _dev(wsum3), torch.empty(1, rows, 1))            # (the source tensor: only its row count is read)
    out, log = _logged(lib, lambda: ops.wsum_finalize(pack, _dev(coef4), _dev(mean), dW))
    torch.cuda.synchronize()
    _ran(log, lc.FINALIZE, wsum.shape[1])
    return dW


@pytest.mark.parametrize("blocks", lc.FINALIZE_BLOCKS)
@pytest.mark.parametrize("rows", lc.FINALIZE_ROWS)
def test_wsum_finalize_on_synthetic_sums(blocks, rows):
    """the 32-slice / 8-unrolled / tail loop at block counts around its edges; columns beyond ws_rows stay untouched"""
    from usip_amd import _lib
    wsum, wsum3, coef4, mean = lo.wsum_synthetic(blocks, 64, rows)
    dW = _finalize(_lib.lib(), wsum, wsum3, coef4, mean, rows, rows + 3)
    _eq(dW[:, :rows], lo.wsum_finalize_ref(wsum, wsum3, coef4, mean, rows), "dW")
    assert _all_nan(dW[:, rows:])


@pytest.mark.parametrize("name", [n for n, c in lc.LAYER_CASES.items() if c["kernel"] == lc.L64WS])
def test_wsum_finalize_on_the_fixtures_own_sums(name):
    from usip_amd import _lib
    fx = lc.layer_case_fixture(name)
    rows = lc.LAYER_CASES[name]["opt"]["ws"]
    _, _, coef4, mean = lo.wsum_synthetic(1, 64, rows, seed=len(name))
    dW = _finalize(_lib.lib(), fx["wsum"], fx["wsum3"], coef4, mean, rows, 8 + 2)
    _eq(dW[:, :rows], lo.wsum_finalize_ref(fx["wsum"], fx["wsum3"], coef4, mean, rows, exact=False), "dW")
    assert _all_nan(dW[:, rows:])


def test_fused_sums_and_finalise_equal_the_producing_layers_own_weight_gradient():
    """(layer_bwd_x2ws_kernel, wsum_finalize_kernel) against ops.mlp_wgrad of the producing layer over (dX, X, S), on a fixture
    whose every product and sum of that layer is exact in fp32 too: all three give the fp64 value"""
    from usip_amd import _lib, ops
    lib = _lib.lib()
    c = dict(name="pair", kernel=lc.L64WS, cin=64, cout=64, nb=2, P=1024, wgs=64, opt=dict(red=True, ws=5))
    fx = lo.layer_fixture(64, 64, 2, 1024, red=True, ws_rows=5, seed=3, w_log2=1)
    coef4, mean, want = lo.producing_layer(fx)
    with _Switches("f32x2"):
        L = _Layer(c, fx)
        got, log = _logged(lib, L.through_ops)
        torch.cuda.synchronize()
    _ran(log, c["kernel"], c["wgs"])
    _check_layer(L, got)
    dWp = _nan(64, 8)
    ops.wsum_finalize(got["red"].wsum, _dev(coef4), _dev(mean), dWp)
    _eq(dWp[:, :5], want, "finalised dW'")
    assert _all_nan(dWp[:, 5:])
    with _Switches("f32"):
        alone = ops.mlp_wgrad(got["dx"], L.wsrc, pro=2, G2=L.x, coef4=_dev(coef4))
        torch.cuda.synchronize()
    _eq(alone, want, "stand-alone dW'")


# ------------------------------------------------------------------------------------------------ zero operands
@pytest.mark.parametrize("name", ["64x64 red second tile in another cloud", "pooled PG group 64, one and two tiles"])
def test_zero_gradient_and_zero_weights_give_exact_zeros(name):
    """An all-zero incoming gradient leaves a zero bound in coef4[4] (scale 2^60), an all-zero W an image scale of 2^60: every
    product is zero times a finite number, every output exactly zero"""
    from usip_amd import _lib
    lib = _lib.lib()
    c = lc.LAYER_CASES[name]
    fx = dict(lc.layer_case_fixture(name))
    coef4 = fx["coef4"].copy()
    coef4[2:] = 0.0
    fx["coef4"] = coef4
    if fx["pool"] is None:
        fx["dZ"] = np.zeros_like(fx["dZ"])
    else:
        fx["pool"] = (np.zeros_like(fx["pool"][0]), fx["pool"][1], fx["pool"][2])
    fx["Wst"] = np.zeros_like(fx["Wst"])
    with _Switches("f32x2"):
        L = _Layer(c, fx)
        got, log = _logged(lib, L.through_ops)
        torch.cuda.synchronize()
    _ran(log, c["kernel"], c["wgs"])
    outs = [got["dx"], L.dw[:, L.wcol:L.wcol + L.cin]] + ([got["sums"], got["maxima"]] if L.red else [])
    for t in outs:
        assert bool(torch.isfinite(t).all()) and not bool(t.any())


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_args(pooled=False, cin=64, cout=64, P=64, red=True, gsum=False, group=32):
    nb, blocks = 1, 256
    a = dict(dZ=None if pooled else _nan(nb, cout, P), Y=_nan(nb, cout, P + 4), coef4=_nan(5, cout),
             pool_dp=_nan(nb, cout, P) if pooled else None, pool_arg=torch.zeros(nb, cout, P, dtype=torch.int32, device=DEV)
             if pooled else None, pool_group=group if pooled else 0, X=_nan(nb, cin, P + 4), x_rows=cin, xcoef=_nan(4, cin),
             planes=_nan(2 * 128 * 128 + 64), dX=_nan(nb, cin, P + 4), dx_rows=cin, workspace=_nan(blocks * cout * cin),
             dW=_nan(cout, cin), lddw=cin, red=_nan(2 * blocks * cin + blocks) if red else None,
             gsum=_nan(2, nb, cin, P) if gsum else None, Cin=cin, Cout=cout, P=P, nb=nb)
    return a


def _call_layer(lib, a, off=None):
    off = off or {}
    p = lambda k: _p(a[k], off.get(k, 0))                        # noqa: E731
    return lib.usip_mlp_layer_backward_x2h_f32(p("dZ"), p("Y"), p("coef4"), p("pool_dp"), p("pool_arg"), a["pool_group"], p("X"),
                                               a["x_rows"], p("xcoef"), p("planes"), p("dX"), a["dx_rows"], p("workspace"),
                                               p("dW"), a["lddw"], p("red"), p("gsum"), a["Cin"], a["Cout"], a["P"], a["nb"], None)


def _call_ws(lib, a, wsrc, ws_rows, wsum, wsum3, off=0):
    p = lambda k: _p(a[k])                                       # noqa: E731
    return lib.usip_mlp_layer_backward_x2h_ws_f32(p("dZ"), p("Y"), p("coef4"), p("X"), a["x_rows"], p("xcoef"), p("planes"),
                                                  p("dX"), a["dx_rows"], p("workspace"), p("dW"), a["lddw"], p("red"),
                                                  _p(wsrc, off), ws_rows, _p(wsum), _p(wsum3), a["Cin"], a["Cout"], a["P"],
                                                  a["nb"], None)


def _refused(lib, call, outs):
    rc, log = _logged(lib, call)
    torch.cuda.synchronize()
    assert rc != 0 and log == [], (rc, log)
    for t in outs:
        if t is not None:
            assert _all_nan(t)


LAYER_REFUSALS = {
    "misaligned dZ": (dict(), dict(off=dict(dZ=4))),
    "misaligned Y": (dict(), dict(off=dict(Y=4))),
    "misaligned X": (dict(), dict(off=dict(X=4))),
    "misaligned dX": (dict(), dict(off=dict(dX=4))),
    "misaligned planes": (dict(), dict(off=dict(planes=4))),
    "P no multiple of 64": (dict(), dict(set=dict(P=32))),
    "x_rows below Cin": (dict(), dict(set=dict(x_rows=63))),
    "dx_rows below Cin": (dict(), dict(set=dict(dx_rows=63))),
    "lddw below Cin": (dict(), dict(set=dict(lddw=63))),
    "pooled with 64 inputs": (dict(pooled=True, red=False), dict()),
    "pooled with 64 inputs, 128 outputs": (dict(pooled=True, cout=128, red=False), dict()),
    "red with a group that is no multiple of 32": (dict(pooled=True, cin=128, cout=128, P=192, group=48), dict()),
    "gsum without red": (dict(pooled=True, cin=128, cout=128, red=False, gsum=True), dict()),
    "gsum unpooled": (dict(gsum=True), dict()),
}


@pytest.mark.parametrize("what", list(LAYER_REFUSALS))
def test_layer_backward_refuses_before_any_launch(what):
    from usip_amd import _lib
    lib = _lib.lib()
    build, change = LAYER_REFUSALS[what]
    a = _refusal_args(**build)
    a.update(change.get("set", {}))
    _refused(lib, lambda: _call_layer(lib, a, change.get("off")), [a["dX"], a["dW"], a["red"], a["gsum"], a["workspace"]])


@pytest.mark.parametrize("what", ["128 outputs", "no source rows", "nine source rows", "misaligned source", "without red"])
def test_ws_entry_refuses_before_any_launch(what):
    from usip_amd import _lib
    lib = _lib.lib()
    a = _refusal_args(cout=128 if what == "128 outputs" else 64, red=what != "without red")
    rows = {"no source rows": 0, "nine source rows": 9}.get(what, 3)
    wsrc, wsum, wsum3 = _nan(1, 9, 64 + 4), _nan(256, 64, 16), _nan(256, 8)
    _refused(lib, lambda: _call_ws(lib, a, wsrc, rows, wsum, wsum3, 4 if what == "misaligned source" else 0),
             [a["dX"], a["dW"], a["red"], wsum, wsum3])


def test_narrow_backward_refuses_red_without_coefficients():
    from usip_amd import _lib
    lib = _lib.lib()
    a = _refusal_args()
    W = _nan(64, 64)
    def call():
        return lib.usip_mlp_narrow_backward_f32(_p(a["dZ"]), _p(a["Y"]), _p(a["coef4"]), _p(a["X"]), 64, None, _p(W), 64,
                                                _p(a["dX"]), 64, _p(a["workspace"]), _p(a["dW"]), 64, _p(a["red"]), 64, 64, 64, 1,
                                                None)
    _refused(lib, call, [a["dX"], a["dW"], a["red"], a["workspace"]])


@pytest.mark.parametrize("blocks,lddw", [(0, 8), (4, 2)])
def test_wsum_finalize_refuses_before_any_launch(blocks, lddw):
    from usip_amd import _lib
    lib = _lib.lib()
    wsum, wsum3, coef4, mean, dW = _nan(4, 64, 16), _nan(4, 8), _nan(4, 64), _nan(64), _nan(64, 8)
    _refused(lib, lambda: lib.usip_mlp_wsum_finalize_f32(_p(wsum), _p(wsum3), blocks, 64, _p(coef4), _p(mean), 3, _p(dW), lddw,
                                                         None), [dW])
