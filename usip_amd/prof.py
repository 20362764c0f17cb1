"""Per-kernel HIP-event timing on the launch stream.

Disabled by default (one boolean test per operator call).  bench.py enables it over the timed
region: every operator wrapper brackets its kernel launch with two events recorded on torch's
current stream -- the stream the kernel is launched on -- and tags the launch with its
ALGORITHMIC work (bytes and/or flops), so that achieved GB/s or TFLOP/s per kernel come from
live measurements of the same run that produces the throughput number.
"""
import ctypes
import re
from collections import defaultdict
from contextlib import contextmanager

import torch

from . import _lib

enabled = False
_only = None                        # when set: only operators whose name starts with this prefix are bracketed
_records = defaultdict(list)        # name -> [(start_event, end_event, bytes, flops)]
_keys = {}                          # name -> rocprof key


def enable(flag: bool = True, only: str = None):
    """only="shared_mlp": bracket just the shared-MLP launches (~80 events instead of ~450 per step)."""
    global enabled, _only
    enabled = flag
    _only = only if flag else None


def reset():
    _records.clear()
    _keys.clear()


def short(name):
    """Kernel name of a rocprofv3 trace (or of the library's launch log) -> the form the traffic tables are keyed by.
    The one copy of this rule: tools/pmc_summary.py imports it."""
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    m = re.match(r"([A-Za-z0-9_:]+)(<[^(]*>)?\(", name)
    if name.startswith("Cijk_"):
        return "rocBLAS " + name[:20]
    return (m.group(1) + (m.group(2) or "")) if m else name[:80]


def _first_launch_key():
    """Key of the first kernel the library launched from this thread since the log was armed; None when there was none."""
    wg = ctypes.c_uint(0)
    name = _lib.lib().usip_launch_log_entry(0, ctypes.byref(wg))
    return None if name is None else "%s |wg=%d" % (short(name.decode()), wg.value)


@contextmanager
def kernel(name: str, nbytes: float = 0.0, flops: float = 0.0, keyed: bool = False, moved: float = 0.0):
    """keyed: record the launch's rocprof key, "<kernel template> |wg=<workgroups>" as tools/pmc_summary.py names launches,
    so that PMC traffic collected in a separate rocprofv3 pass can be attached to this operator.  The key is not worked
    out here: the library's launch log (usip_launch_log, armed over the bracket) says which kernel the call launched FIRST
    and with how many workgroups.  A bracket that launched nothing leaves no key.
    moved: bytes the launch moves INTO its CUs by construction, L2-served re-reads included (the split GEMMs re-read
    their weight planes for every position tile) -- what the per-CU memory path (~25 GB/s) has to carry."""
    if not enabled or (_only is not None and not name.startswith(_only)):
        yield
        return
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    if keyed:
        _lib.lib().usip_launch_log(1)
    s.record()                      # current stream == launch stream of the wrapped kernel
    yield
    e.record()
    if keyed:                       # (behind the closing event: resolving the name takes host time)
        key = _first_launch_key()
        _lib.lib().usip_launch_log(0)
        if key is not None:
            _keys[name] = key
    _records[name].append((s, e, nbytes, flops, moved))


def summary():
    """{name: dict(calls, total_ms, avg_us, bytes_per_call, flops_per_call, GBps, TFLOPs)} (synchronises)."""
    torch.cuda.synchronize()
    out = {}
    for name, recs in _records.items():
        ms = [r[0].elapsed_time(r[1]) for r in recs]
        tot = sum(ms)
        nb = sum(r[2] for r in recs) / len(recs)
        fl = sum(r[3] for r in recs) / len(recs)
        avg_s = tot / len(recs) * 1e-3
        out[name] = dict(rocprof_key=_keys.get(name), calls=len(recs), total_ms=tot, avg_us=avg_s * 1e6, bytes_per_call=nb,
                         moved_per_call=sum(r[4] for r in recs) / len(recs),
                         flops_per_call=fl, GBps=(nb / avg_s / 1e9) if avg_s > 0 else 0.0,
                         TFLOPs=(fl / avg_s / 1e12) if avg_s > 0 else 0.0)
    return out
