"""What the GPU tests of the shared-MLP product family share: device copies, the launch log, the switches of a case."""
import ctypes

import numpy as np
import torch

DEV = "cuda:0"
KNOBS = ("gemm_split3", "x2_direct", "r5_forms", "x3_gemm_tile")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _logged(lib, call):
    """-> (call(), [(kernel name, workgroups)] of what the library launched for it)"""
    lib.usip_launch_log(1)
    try:
        out, got, wg = call(), [], ctypes.c_uint(0)
        while (name := lib.usip_launch_log_entry(len(got), ctypes.byref(wg))) is not None:
            got.append((name.decode(), int(wg.value)))
    finally:
        lib.usip_launch_log(0)
    return out, got


def _ran(got, kernel, wgs):
    hits = [(n, w) for n, w in got if "::" + kernel + "(" in n]
    assert hits, (kernel, got)
    assert hits[-1][1] == wgs, (kernel, wgs, got)


# index of each knob for usip_tuning_value: its place in host_cpu.cpp's name table
KNOB_INDEX = {"x3_wgrad_tile": 2, "x3_gemm_tile": 3, "gemm_split3": 4, "x2_direct": 6, "r5_forms": 7}


class _Switches:
    """Matmul mode, tuning knobs, NARROW_FWD, POOL_GRAD_FOLD and PLANES_CACHE of one case.  Every listed knob is SET (0 unless the
    case names a value), so a case does not depend on what the process had; on exit everything goes back to what it was."""

    def __init__(self, mode, knobs=None, cache=False, narrow=True, fold=True):
        self.mode, self.knobs, self.cache, self.narrow, self.fold = mode, dict(knobs or {}), cache, narrow, fold

    def __enter__(self):
        from usip_amd import _lib, ops
        lib = _lib.lib()
        assert set(self.knobs) <= set(KNOBS)
        self.prev_knobs = {k: int(lib.usip_tuning_value(KNOB_INDEX[k])) for k in KNOBS}
        self.prev = (ops.set_matmul_mode(self.mode), ops.NARROW_FWD, ops.PLANES_CACHE, ops.POOL_GRAD_FOLD)
        ops.NARROW_FWD, ops.POOL_GRAD_FOLD = self.narrow, self.fold
        ops.PLANES_CACHE = {} if self.cache else None
        for k in KNOBS:
            assert lib.usip_set_tuning(k.encode(), int(self.knobs.get(k, 0))) == 0
        return self

    def __exit__(self, *exc):
        from usip_amd import _lib, ops
        for k, v in self.prev_knobs.items():
            _lib.lib().usip_set_tuning(k.encode(), v)
        ops.set_matmul_mode(self.prev[0])
        ops.NARROW_FWD, ops.PLANES_CACHE, ops.POOL_GRAD_FOLD = self.prev[1], self.prev[2], self.prev[3]
        return False
