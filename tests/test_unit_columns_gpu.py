"""csrc/unit_columns.hip against its host twin, BIT FOR BIT (NaN where NaN), forward and backward, on the case grid of
tests/test_unit_columns_cpu.py -- C and M at and around the wave width, one and three batch elements, a zero column, NaN and
Inf in one column, a column of 1e30 -- and on a launch of more positions than one sweep of the grid covers.  The launch log
names the two kernels."""
import ctypes

import numpy as np
import pytest
import torch

from gemm_gpu_helpers import DEV, _logged
from test_unit_columns_cpu import EPS, case, cases, same_bits, twin

pytestmark = pytest.mark.gpu


def _device(x, g, eps=EPS):
    from usip_amd import _lib, ops
    xd, gd = torch.from_numpy(x).to(DEV), torch.from_numpy(g).to(DEV)
    (out, n), fwd = _logged(_lib.lib(), lambda: ops.unit_columns(xd, eps))
    dx, bwd = _logged(_lib.lib(), lambda: ops.unit_columns_backward(gd, xd, n, eps))
    torch.cuda.synchronize()
    return (out.cpu().numpy(), n.cpu().numpy(), dx.cpu().numpy()), fwd, bwd


def _equal(got, want, what):
    for a, b, part in zip(got, want, ("out", "norm", "dx")):
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, part)
        assert same_bits(np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0)), (what, part)


@pytest.mark.parametrize("name", sorted(cases()))
def test_device_equals_twin_bit_for_bit(name):
    x, g = cases()[name]
    got, fwd, bwd = _device(x, g)
    _equal(got, twin(x, g), name)
    rows = x.shape[0] * x.shape[2]
    assert len(fwd) == 1 and "unit_columns_kernel" in fwd[0][0] and fwd[0][1] == (rows + 63) // 64, fwd
    assert len(bwd) == 1 and "unit_columns_backward_kernel" in bwd[0][0] and bwd[0][1] == (rows + 63) // 64, bwd


def test_more_positions_than_one_sweep_of_the_grid():
    """65536 workgroups of 64 cover 2^22 positions; the rest is the kernels' loop"""
    M = (1 << 22) + 65
    x, g = case(1, 2, M, 9)
    got, fwd, bwd = _device(x, g)
    _equal(got, twin(x, g, threads=16), "beyond the grid")
    assert fwd[0][1] == 65536 and bwd[0][1] == 65536


def test_eps_zero_and_the_autograd_function():
    from usip_amd import functional as Fh
    x, g = case(3, 65, 63, 2)
    _equal(_device(x, g, 0.0)[0], twin(x, g, 0.0), "eps 0")
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = Fh.unit_columns(xd, EPS)
    out.backward(torch.from_numpy(g).to(DEV))
    want = twin(x, g)
    assert same_bits(out.detach().cpu().numpy(), want[0]) and same_bits(xd.grad.cpu().numpy(), want[2])
    # a non-contiguous input and gradient are taken as their contiguous copies
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(DEV).transpose(1, 2).requires_grad_(True)
    out = Fh.unit_columns(xt, EPS)
    out.backward(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 2, 1))).to(DEV).transpose(1, 2))
    assert same_bits(out.detach().cpu().numpy(), want[0]) and same_bits(xt.grad.cpu().numpy(), want[2])


def test_device_entry_points_refuse_what_the_twin_refuses():
    from usip_amd import _lib, ops
    lib = _lib.lib()
    x = torch.zeros(2, 3, 4, device=DEV)
    n = torch.zeros(2, 4, device=DEV)
    out = torch.full_like(x, 7.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    for B, C, M, eps in ((-1, 3, 4, EPS), (2, -1, 4, EPS), (2, 3, -1, EPS), (2, 3, 4, -1.0), (2, 3, 4, float("nan"))):
        assert lib.usip_unit_columns_f32(p(x), B, C, M, eps, p(out), p(n), None) == -1
        assert lib.usip_unit_columns_backward_f32(p(x), p(x), p(n), B, C, M, eps, p(out), None) == -1
    assert lib.usip_unit_columns_f32(None, 2, 3, 4, EPS, p(out), p(n), None) == -1
    assert lib.usip_unit_columns_backward_f32(p(x), p(x), p(n), 2, 3, 4, EPS, None, None) == -1
    _, got = _logged(lib, lambda: (lib.usip_unit_columns_f32(p(x), 0, 3, 4, EPS, p(out), p(n), None),
                                   lib.usip_unit_columns_backward_f32(p(x), p(x), p(n), 2, 3, 0, EPS, p(out), None)))
    torch.cuda.synchronize()
    assert got == [] and bool((out == 7.0).all())                     # zero rows: USIP_OK, no launch
    o, nn = ops.unit_columns(torch.zeros(0, 3, 4, device=DEV))
    assert o.shape == (0, 3, 4) and nn.shape == (0, 4)
    with pytest.raises(RuntimeError):
        ops.unit_columns(x.double())
    with pytest.raises(RuntimeError):
        ops.unit_columns_backward(x, x, n[:, :3].contiguous())
