"""Every form of the shared-MLP weight gradient, bit for bit (ops.mlp_wgrad: csrc/shared_mlp.hip wgrad_kernel,
shared_mlp_bf16.hip wgrad_bf16_kernel with one and three planes, shared_mlp_x3.hip wgrad_x3_kernel / wgrad_x2l_kernel).

Operands from tests/gemm_oracle.py::wgrad_fixture: few nonzero values over thousands of positions, every element exact in the
planes its form keeps, per position at most one operand with low planes, sum |products| below 2^24 units -- so the slicing,
the partial tiles and their fixed-order sum cannot change a bit and dW must EQUAL the fp64 product.  No tolerance appears
in this file.  Each case asserts from the launch log which instantiation ran, with the workgroup count its segment plan
(gemm_oracle.wgrad_plan / wgrad_x3_plan, restated from the library) gives."""
import pytest
import torch

import gemm_cases as gc
from gemm_gpu_helpers import DEV, _Switches, _dev, _logged, _ran

pytestmark = pytest.mark.gpu


def _call(c, fx, out=None, coloff=0):
    from usip_amd import ops
    kw = dict(pro=c["pro"], G2=_dev(fx["G2"]), coef4=_dev(fx["coef4"]), out=out, coloff=coloff)
    if fx["xcoef"] is not None:
        kw["xcoef"] = _dev(fx["xcoef"])
        ops.declare_samples(kw["xcoef"], c["nb"] * c["P"])
    if c["pro"] == 3:
        dp, arg, g = fx["pool"]
        kw["pool"] = (_dev(dp), _dev(arg), g)
    G, X = _dev(fx["G"]), _dev(fx["X"])
    return lambda: ops.mlp_wgrad(G, X, **kw)


@pytest.mark.parametrize("name", list(gc.WGRAD_CASES))
def test_wgrad_form_equals_the_exact_product(name):
    from usip_amd import _lib
    lib = _lib.lib()
    c = gc.WGRAD_CASES[name]
    o = c["opt"]
    fx = gc.wgrad_case_fixture(name)
    M, N = c["M"], c["N"]
    assert int(lib.usip_mlp_wgrad_workspace(M, N, c["P"], c["nb"])) >= c["nb"] * c["segs"] * M * N
    coloff = int(o.get("coloff", 0))
    out = torch.full((M, N + coloff + 2), float("nan"), device=DEV) if coloff else None
    with _Switches(c["mode"], o.get("knobs")):
        dW, got = _logged(lib, _call(c, fx, out, coloff))
        torch.cuda.synchronize()
    _ran(got, c["kernel"], c["wgs"])
    want = _dev(fx["want"])
    res = dW if out is None else out[:, coloff:coloff + N]
    assert torch.equal(res, want), "%d of %d weight gradients differ" % (int((res != want).sum()), want.numel())
    if out is not None:
        assert bool(torch.isnan(out[:, :coloff]).all()) and bool(torch.isnan(out[:, coloff + N:]).all())


@pytest.mark.parametrize("name", ["f32 128 tiles, many slices, short last segment", "x3 256 tiles", "x2l pro2"])
def test_deferred_reduction_gives_the_same_bits(name):
    """wgrad_defer(True, device) ... wgrad_flush: the recorded fixed-order sum lands the same bits as the immediate one"""
    from usip_amd import _lib, ops
    lib = _lib.lib()
    c = gc.WGRAD_CASES[name]
    fx = gc.wgrad_case_fixture(name)
    M, N = c["M"], c["N"]
    out = torch.full((M, N + 4), float("nan"), device=DEV)
    with _Switches(c["mode"], c["opt"].get("knobs")):
        call = _call(c, fx, out, 1)
        ops.wgrad_defer(True, DEV)
        try:
            _, got = _logged(lib, call)
            torch.cuda.synchronize()
            assert not any("wgrad_reduce" in n for n, _ in got), got      # recorded, not launched
            assert bool(torch.isnan(out).all())
            assert ops.wgrad_flush(DEV) >= 1
            torch.cuda.synchronize()
        finally:
            ops.wgrad_defer(False)
    _ran(got, c["kernel"], c["wgs"])
    assert torch.equal(out[:, 1:1 + N], _dev(fx["want"]))
    assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(out[:, 1 + N:]).all())
