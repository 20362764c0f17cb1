"""The unchanged GEMM and fused layer-backward forms at a row-bias / pooled group of 448 (tests/wide_form_cases.py), judged as
tests/test_gemm_forms_gpu.py and tests/test_layer_bwd_forms_gpu.py judge their cases: operands for which the fp64 result is an
fp32 number whatever the accumulation order, torch.equal, and the instantiation and workgroup count from the launch log.  No
tolerance appears in this file."""
import pytest
import torch

import gemm_oracle as go
import wide_form_cases as wc
from gemm_gpu_helpers import _Switches, _dev, _logged, _ran
from test_layer_bwd_forms_gpu import _check_layer, _Layer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(wc.WIDE_GEMM_CASES))
def test_forward_form_takes_a_row_bias_per_448_positions(name):
    from usip_amd import _lib, ops
    lib = _lib.lib()
    c = wc.WIDE_GEMM_CASES[name]
    o = c["opt"]
    fx = wc.wide_gemm_fixture(name)
    nb, K, M, P = c["nb"], c["K"], c["M"], c["P"]
    assert fx["rb_group"] == wc.GROUP and P % wc.GROUP == 0 and fx["record"]["rb_straddles_tile"]
    At, X, coef = _dev(go.at_storage(fx["A"], M, 0)), _dev(fx["X"]), _dev(fx["coef"])
    with _Switches(c["mode"], o.get("knobs")):
        ops.declare_samples(coef, nb * P)                      # hand-built statistics: taken over this launch's samples
        res, got = _logged(lib, lambda: ops.mlp_gemm(At, X, bias=_dev(fx["bias"]), want_stats=True, pro=1, coef=coef, M=M,
                                                     rowbias=_dev(fx["rowbias"]), rb_group=wc.GROUP))
        torch.cuda.synchronize()
    _ran(got, c["kernel"], c["wgs"])
    want, st = _dev(fx["want"]), _dev(fx["stats"])
    assert res[0].shape == want.shape and res[1].shape == st.shape, (res[0].shape, res[1].shape, st.shape)
    assert torch.equal(res[0], want), "%d of %d outputs differ" % (int((res[0] != want).sum()), want.numel())
    assert torch.equal(res[1], st), "%d of %d statistics partials differ" % (int((res[1] != st).sum()), st.numel())


@pytest.mark.parametrize("name", list(wc.WIDE_LAYER_CASES))
def test_pooled_layer_backward_takes_a_group_of_448(name):
    from usip_amd import _lib
    lib = _lib.lib()
    c = wc.WIDE_LAYER_CASES[name]
    fx = wc.wide_layer_fixture(name)
    assert fx["pool"][2] == wc.GROUP
    with _Switches("f32x2"):
        L = _Layer(c, fx)
        got, log = _logged(lib, L.through_ops)
        torch.cuda.synchronize()
    _ran(log, c["kernel"], c["wgs"])
    assert sum(1 for n, _ in log if "layer_bwd_x2" in n) == 1, log
    _check_layer(L, got)
