"""The unit normalisation's host twin (csrc/unit_columns_cpu.cpp over csrc/unit_math.h; include/usip_hip.h f-25) against the
numpy restatement of the contract (tests/indoor_oracle.py: one IEEE operation at a time in the contract's order, so the
comparison is EQUALITY), against torch under double autograd at 1e-5, and a stand-alone sanitizer build.  The device is held to
this twin bit for bit in tests/test_unit_columns_gpu.py, which borrows `cases`."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import indoor_oracle as io_
from conftest import ROOT
from usip_amd import _lib, ops

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")
EPS = 1e-5
GRID = list(itertools.product((1, 3), (1, 3, 64, 65, 130), (1, 63, 64, 65, 130)))          # (B, C, M)


def case(B, C, M, seed=0):
    """-> (x, grad) f32 [B,C,M]"""
    g = np.random.default_rng(1000 * B + 10 * C + M + seed)
    return g.standard_normal((B, C, M)).astype(np.float32), g.standard_normal((B, C, M)).astype(np.float32)


def special_cases():
    """name -> (x, grad): a zero column, a NaN in one column only, a column of 1e30, an Inf"""
    out = {}
    x, g = case(2, 5, 7)
    x[1, :, 3] = 0.0
    out["zero column"] = (x, g)
    x, g = case(2, 5, 7, 1)
    x[0, 2, 4] = np.nan
    out["nan in one column"] = (x, g)
    x, g = case(1, 6, 5, 2)
    x[0, :, 1] = 1e30
    out["column of 1e30"] = (x, g)
    x, g = case(1, 4, 3, 3)
    x[0, 1, 2] = np.inf
    out["inf in one column"] = (x, g)
    x, g = case(1, 4, 3, 4)
    g[0, 0, 0] = np.nan
    out["nan gradient"] = (x, g)
    return out


def cases():
    out = {"B%d C%d M%d" % k: case(*k) for k in GRID}
    out.update(special_cases())
    return out


def twin(x, g, eps=EPS, threads=1):
    xt, gt = torch.from_numpy(x), torch.from_numpy(g)
    out, n = ops.unit_columns_cpu(xt, eps, threads)
    dx = ops.unit_columns_backward_cpu(gt, xt, n, eps, threads)
    return out.numpy(), n.numpy(), dx.numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(cases()))
def test_twin_equals_the_restated_contract(name):
    x, g = cases()[name]
    out, n, dx = twin(x, g)
    want_out, want_n = io_.unit_forward(x, EPS)
    want_dx = io_.unit_backward(g, x, want_n, EPS)
    # (NaN payloads are not part of the contract: NaN where NaN, every other bit equal)
    for got, want, what in ((out, want_out, "out"), (n, want_n, "norm"), (dx, want_dx, "dx")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, what)
        assert same_bits(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)), (name, what)


def test_zero_nan_and_huge_columns():
    sp = special_cases()
    x, g = sp["zero column"]
    out, n, dx = twin(x, g)
    assert n[1, 3] == 0.0 and (out[1, :, 3] == 0.0).all()
    assert same_bits(dx[1, :, 3], (g[1, :, 3].astype(np.float64) / np.float64(np.float32(EPS))).astype(np.float32))  # torch's zero sub-gradient
    x, g = sp["nan in one column"]
    out, n, dx = twin(x, g)
    bad = np.zeros(x.shape, bool)
    bad[0, :, 4] = True
    assert np.isnan(out[bad]).all() and np.isnan(dx[bad]).all() and np.isnan(n[0, 4])
    assert np.isfinite(out[~bad]).all() and np.isfinite(dx[~bad]).all()
    x, g = sp["column of 1e30"]
    out, n, dx = twin(x, g)
    assert np.isfinite(out).all() and np.isfinite(dx).all() and np.isfinite(n).all()
    assert abs(float(n[0, 1]) / (1e30 * np.sqrt(6.0)) - 1.0) < 1e-6
    np.testing.assert_allclose(np.sqrt((out[0, :, 1].astype(np.float64) ** 2).sum()), 1.0, rtol=1e-6)


def test_thread_counts_agree():
    x, g = case(3, 65, 130)
    ref = twin(x, g, threads=1)
    for threads in (2, 3, 7, 64, 1000):
        for a, b in zip(ref, twin(x, g, threads=threads)):
            assert same_bits(a, b), threads


def test_twin_is_within_the_bar_of_torch_under_double_autograd():
    for B, C, M in ((3, 64, 65), (1, 130, 63), (2, 3, 130)):
        x, g = case(B, C, M, 5)
        out, _, dx = twin(x, g)
        xd = torch.from_numpy(x).double().requires_grad_(True)
        ref = xd / (torch.norm(xd, dim=1, keepdim=True) + EPS)
        ref.backward(torch.from_numpy(g).double())
        assert np.abs(out - ref.detach().numpy()).max() / np.abs(ref.detach().numpy()).max() <= 1e-5
        assert np.abs(dx - xd.grad.numpy()).max() / np.abs(xd.grad.numpy()).max() <= 1e-5


def test_autograd_function_on_host_tensors():
    from usip_amd import functional as Fh
    x, g = case(2, 9, 11)
    xt = torch.from_numpy(x).requires_grad_(True)
    out = Fh.unit_columns(xt, EPS, num_threads=2)
    out.backward(torch.from_numpy(g))
    want = twin(x, g)
    assert same_bits(out.detach().numpy(), want[0]) and same_bits(xt.grad.numpy(), want[2])


def test_every_argument_limit():
    lib = _lib.lib()
    x, g = case(2, 3, 4)
    X, G = torch.from_numpy(x), torch.from_numpy(g)
    out, n, dx = torch.zeros_like(X), torch.zeros(2, 4), torch.zeros_like(X)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    ok = lib.usip_unit_columns_f32_cpu
    okb = lib.usip_unit_columns_backward_f32_cpu
    assert ok(p(X), 2, 3, 4, EPS, p(out), p(n), 1) == 0
    assert okb(p(G), p(X), p(n), 2, 3, 4, EPS, p(dx), 1) == 0
    assert ok(p(X), 2, 3, 4, 0.0, p(out), p(n), 1) == 0               # eps = 0 is inside the limits
    # zero rows: nothing to do, and nothing is touched
    out.fill_(7.0)
    for B, C, M in ((0, 3, 4), (2, 3, 0), (0, 0, 0)):
        assert ok(p(X), B, C, M, EPS, p(out), p(n), 1) == 0 and okb(p(G), p(X), p(n), B, C, M, EPS, p(dx), 1) == 0
    assert (out == 7.0).all()
    # no channels: the norm of nothing is 0
    n.fill_(5.0)
    assert ok(p(X), 2, 0, 4, EPS, p(out), p(n), 1) == 0 and (n == 0.0).all()
    for B, C, M, eps in ((-1, 3, 4, EPS), (2, -1, 4, EPS), (2, 3, -1, EPS), (2, 3, 4, -1e-5), (2, 3, 4, float("nan"))):
        assert ok(p(X), B, C, M, eps, p(out), p(n), 1) == -1, (B, C, M, eps)
        assert okb(p(G), p(X), p(n), B, C, M, eps, p(dx), 1) == -1, (B, C, M, eps)
    assert ok(None, 2, 3, 4, EPS, p(out), p(n), 1) == -1 and ok(p(X), 2, 3, 4, EPS, None, p(n), 1) == -1
    assert ok(p(X), 2, 3, 4, EPS, p(out), None, 1) == -1
    for args in ((None, p(X), p(n), p(dx)), (p(G), None, p(n), p(dx)), (p(G), p(X), None, p(dx)), (p(G), p(X), p(n), None)):
        assert okb(args[0], args[1], args[2], 2, 3, 4, EPS, args[3], 1) == -1
    # the wrappers refuse what the entry points would misread
    with pytest.raises(RuntimeError):
        ops.unit_columns_cpu(X.double())
    with pytest.raises(RuntimeError):
        ops.unit_columns_cpu(X[:, :, ::2])
    with pytest.raises(RuntimeError):
        ops.unit_columns_cpu(X, -1.0)
    with pytest.raises(RuntimeError):
        ops.unit_columns_backward_cpu(G[:1], X, n)
    with pytest.raises(RuntimeError):
        ops.unit_columns_backward_cpu(G, X, n[:, :3].contiguous())
    with pytest.raises(RuntimeError):
        ops.unit_columns(X)                                           # a host tensor at the device wrapper


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/unit_columns_cpu.cpp.  It links nothing of the package and is never loaded
    into Python."""
    exe = str(tmp_path / "unit_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", os.path.join(ROOT, "tests", "unit_sanitize_main.cpp"),
                    os.path.join(ROOT, "usip_amd", "csrc", "unit_columns_cpu.cpp"), "-o", exe, "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
