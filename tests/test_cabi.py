"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/usip_hip.h declares, and the host-side mirror of the reference interface behaves like
the reference's (names, argument meaning, error behaviour).  No device compute here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "usip_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(usip_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from usip_amd import _lib
    lib = _lib.lib()
    declared = _declared_symbols()
    assert "usip_ball_query_f32" in declared and "usip_index_max_f32" in declared
    for name in declared:
        assert hasattr(lib, name), "libusip_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, "no ctypes signature for %s" % name
    assert b"gfx950" in lib.usip_version()
    # the signatures are read from the header (usip_amd/_lib.py): the reader neither misses nor invents a declaration
    assert set(_lib.SIGNATURES) == set(declared)


_V, _I, _D, _LL, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong, ctypes.c_uint64
# written by hand from include/usip_hip.h, one row for each kind of type the reader maps
_PINNED_SIGNATURES = {
    "usip_version": ([], ctypes.c_char_p),                                                          # const char* returned
    "usip_launch_log_entry": ([_I, ctypes.POINTER(ctypes.c_uint)], ctypes.c_char_p),                # unsigned*
    "usip_index_max_geometry": ([_I] * 4 + [ctypes.POINTER(ctypes.c_int)] * 3, _I),                 # int*
    "usip_ball_query_f32": ([_V, _V, ctypes.c_float, _I, _I, _I, _I, _V], _I),                      # float
    "usip_iss_saliency_f32": ([_V, _V, _V, _I, _I, _D, _D, _D, _I, _V, _V, _V, _V], _I),            # double
    "usip_nearest_workspace": ([_I, _I, _I], _LL),                                                  # long long returned
    "usip_pairs_build_f32": ([_V, _V, _V, _I, _V, _I, _LL, _U64, _U64, _LL, _V, _V, _V], _I),       # uint64_t, struct*
    "usip_mlp_split3_multi_f32": ([_V, _I, _I, _V], _I),
}


@pytest.mark.parametrize("name", sorted(_PINNED_SIGNATURES))
def test_signatures_read_from_the_header_match_pinned_rows(name):
    from usip_amd import _lib
    assert _lib.SIGNATURES[name] == _PINNED_SIGNATURES[name]


def test_struct_layouts_read_from_the_header_are_the_compilers(tmp_path):
    """sizeof and every field's offset and size of every struct in _lib.STRUCTS, against a C program that includes the header
    (the host C compiler oracle/Makefile uses; a missing compiler fails)."""
    from usip_amd import _lib
    assert len(_lib.STRUCTS) == 8
    lines, expected = [], []
    for name, cls in _lib.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        expected.append("%s %d" % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (name, field, name, field, name, field))
            expected.append("%s.%s %d %d" % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "usip_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)]).decode().split("\n")[:-1] == expected
    # a nested struct is the class already built, so ops.PairsRecipeC() can be assigned to recipe.cloud
    assert dict(_lib.STRUCTS["usip_desc_pairs_recipe"]._fields_)["cloud"] is _lib.STRUCTS["usip_pairs_recipe"]


_SYNTHETIC_HEADER = """
/* no declaration: int usip_x(int a); */
#define USIP_SOMETHING 3
typedef struct usip_inner { int a, b; const float* p; double* q[2]; } usip_inner;
typedef struct usip_outer {
    usip_inner in;      // nested: int usip_y(void);
    long long n; unsigned u;
} usip_outer;
const char* usip_name(void);
int usip_three(const float* x,
               int32_t* idx[2],
               const usip_outer* o, uint64_t seed);
"""


def test_header_reader_on_synthetic_text():
    from usip_amd import _lib
    structs, signatures = _lib.read_header(_SYNTHETIC_HEADER)
    assert list(structs) == ["usip_inner", "usip_outer"]
    assert structs["usip_inner"]._fields_ == [("a", _I), ("b", _I), ("p", _V), ("q", _V * 2)]
    assert structs["usip_outer"]._fields_ == [("in", structs["usip_inner"]), ("n", _LL), ("u", ctypes.c_uint)]
    assert signatures == {"usip_name": ([], ctypes.c_char_p), "usip_three": ([_V, _V * 2, _V, _U64], _I)}
    # what the reader does not know raises and quotes the declaration: it never falls back to int
    for bad, quoted in (("int usip_bad(size_t n);", "size_t n"), ("size_t usip_bad(int n);", "size_t usip_bad"),
                        ("typedef struct s { short a; } s;", "short a"), ("typedef int usip_t;", "typedef int usip_t"),
                        ("int usip_bad(float** x);", "float** x"), ("int usip_bad(int);", "int")):
        with pytest.raises(ValueError, match=re.escape(quoted)):
            _lib.read_header(_SYNTHETIC_HEADER + bad)


def test_abi_number_is_the_headers():
    from usip_amd import _lib
    text = open(os.path.join(ROOT, "include", "usip_hip.h")).read()
    abi = int(re.search(r"^#define\s+USIP_ABI\s+(\d+)", text, re.M).group(1))
    assert _lib.ABI == abi
    assert _lib.lib().usip_version() == b"usip_hip 0.5 gfx950 abi=%d flags=no-contract,no-fast-math,no-slp" % abi


# (channel rows, prefetch depth, threads) for the knob triples (ch, u, th) in (1, 2, 4, 8) x (1, 2, 4) x (256, 512, 1024), in
# that order -- recorded from the Python function ops.index_max_geometry was before the library answered the question; the
# three shapes of test_native_ops_gpu.py::test_index_max_launch_geometries_agree all give this table
_INDEX_MAX_GEOMETRIES = [
    (1, 1, 256), (1, 1, 512), (1, 1, 1024), (1, 2, 256), (1, 2, 512), (1, 2, 1024), (1, 4, 256), (1, 2, 512), (1, 2, 1024),
    (2, 1, 256), (2, 1, 512), (2, 1, 1024), (2, 2, 256), (2, 2, 512), (2, 2, 1024), (2, 4, 256), (2, 2, 512), (2, 2, 1024),
    (4, 1, 256), (4, 1, 512), (4, 1, 1024), (4, 2, 256), (4, 2, 512), (4, 2, 1024), (4, 4, 256), (4, 2, 512), (4, 2, 1024),
    (8, 1, 256), (8, 1, 512), (8, 1, 1024), (8, 2, 256), (8, 2, 512), (8, 2, 1024), (8, 2, 256), (8, 2, 512), (8, 2, 1024)]


def test_index_max_geometry_is_the_launchers_own_choice():
    """ops.index_max_geometry asks the library (usip_index_max_geometry, the function the launcher itself calls) and
    returns what its Python predecessor returned: the sweep of test_index_max_launch_geometries_agree and bench.py's two
    stand-alone shapes with the knobs at rest."""
    import itertools
    from usip_amd import _lib, ops
    lib = _lib.lib()
    try:
        for shape in [(2, 64, 16384, 512), (3, 8, 5000, 37), (1, 16, 1028, 5)]:
            got = []
            for ch, u, th in itertools.product((1, 2, 4, 8), (1, 2, 4), (256, 512, 1024)):
                lib.usip_set_tuning(b"index_max_ch", ch)
                lib.usip_set_tuning(b"index_max_unroll", u)
                lib.usip_set_tuning(b"index_max_threads", th)
                got.append(ops.index_max_geometry(*shape))
            assert got == _INDEX_MAX_GEOMETRIES, shape
    finally:
        for knob in (b"index_max_ch", b"index_max_unroll", b"index_max_threads"):
            lib.usip_set_tuning(knob, 0)
    assert ops.index_max_geometry(16, 64, 16384, 512) == (2, 2, 256)
    assert ops.index_max_geometry(16, 128, 16384, 512) == (2, 2, 256)


def test_dropin_modules_have_reference_entry_points():
    import usip_amd
    im, bq = usip_amd.install()
    import index_max
    import ball_query
    assert index_max is im and ball_query is bq
    for fn in ("forward_cpu", "forward_multi_thread_cpu", "forward_cuda", "forward_cuda_shared_mem"):
        assert callable(getattr(index_max, fn))          # index_max.cpp:154-159
    for fn in ("forward_cuda", "forward_cuda_shared_mem"):
        assert callable(getattr(ball_query, fn))         # ball_query.cpp:45-48


def test_device_entry_points_take_host_tensors_to_the_host_twins_and_never_mix():
    """"`forward_cuda_shared_mem` of both modules accepts CPU tensors so networks.py runs on CPU unchanged"
    (BASELINE configs[0]).  ALL tensor arguments on the host -> the product's own host twins (csrc/host_cpu.cpp; never
    oracle/); a host/device mix or a wrong dtype is still the reference's CHECK_INPUT RuntimeError
    (index_max.cpp:119-121, ball_query.cpp:10-12); the tensor-level device wrappers (usip_amd.ops) refuse host tensors."""
    import usip_amd
    from usip_amd import ops
    im, bq = usip_amd.install()
    g = load_golden("index_max_cases.npz")
    d, i, K = torch.from_numpy(g["ties_data"]), torch.from_numpy(g["ties_index"]), int(g["ties_K"])
    for fn in (im.forward_cuda_shared_mem, im.forward_cuda):
        out = fn(d, i, K)
        assert out.dtype == torch.int32 and not out.is_cuda and np.array_equal(out.numpy(), g["ties_out"])
    # strided views, as networks.py may hand over: read through their strides like the reference's accessor
    wide = torch.zeros(d.shape[0], d.shape[1], 2 * d.shape[2])
    wide[:, :, ::2] = d
    assert np.array_equal(im.forward_cuda_shared_mem(wide[:, :, ::2], i, K).numpy(), g["ties_out"])
    gd = load_golden("dist_ball_cases.npz")
    dist = torch.from_numpy(gd["dist"])
    for fn in (bq.forward_cuda_shared_mem, bq.forward_cuda):
        out = fn(dist, float(gd["radius"]), int(gd["K"]))
        assert out.dtype == torch.int32 and np.array_equal(out.numpy(), gd["ball_idx_unpinned"])
    with pytest.raises(RuntimeError, match="int32|Int"):
        im.forward_cuda_shared_mem(d, i.long(), K)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.index_max(d, i, K)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.ball_query(dist, 0.5, 4)


@pytest.mark.parametrize("tag", ["random", "ties", "floor", "empty", "nan", "tiny", "n_lt_wave"])
@pytest.mark.parametrize("threads", [1, 3])
def test_host_entry_points_match_reference_golden(tag, threads):
    """index_max.forward_cpu / forward_multi_thread_cpu twins against vectors produced by the
    reference's own C++."""
    import usip_amd
    im, _ = usip_amd.install()
    g = load_golden("index_max_cases.npz")
    d, i, K = torch.from_numpy(g[tag + "_data"]), torch.from_numpy(g[tag + "_index"]), int(g[tag + "_K"])
    out = im.forward_cpu(d, i, K) if threads == 1 else im.forward_multi_thread_cpu(d, i, K, threads)
    assert out.dtype == torch.int32
    assert np.array_equal(out.numpy(), g[tag + "_out"])


def test_ball_front_end_host_twins_match_oracle_and_fixture():
    """BASELINE configs[0] (ModelNet40 detector, N=1024, M=64, batch 2 on PyTorch CPU): the Ball front end's two operators
    through the product's own host twins (usip_pairwise_dist_f32_cpu, usip_ball_query_f32_cpu) -- distances bit-identical
    to torch.norm on the pinned platform, rows equal to the C oracle's and to the committed fixture."""
    import usip_amd
    from oracle import native
    from usip_amd import ops, synth
    _, bq = usip_amd.install()
    g = load_golden("dist_ball_cases.npz")
    x, node = torch.from_numpy(g["x"]), torch.from_numpy(g["node"])
    dist = ops.pairwise_dist_cpu(node, x)
    assert np.array_equal(dist.numpy(), g["dist"])
    out = bq.forward_cpu(dist, float(g["radius"]), int(g["K"]))
    assert out.dtype == torch.int32 and np.array_equal(out.numpy(), g["ball_idx_unpinned"])
    b = synth.make_pair_batch(11, 2, 1024, 64, 3, "sphere")            # configs[0] shapes
    x, node = torch.from_numpy(b["src_pc"]), torch.from_numpy(b["src_node"])
    ref = torch.norm(node.unsqueeze(3) - x.unsqueeze(2), dim=1).contiguous()
    dist = ops.pairwise_dist_cpu(node, x)
    assert torch.equal(dist, ref)
    for radius, K in ((0.2, 64), (0.05, 32), (5.0, 8)):                # partially filled, empty and full balls
        assert np.array_equal(bq.forward_cpu(dist, radius, K).numpy(), native.ball_query(dist.numpy(), radius, K))
    with pytest.raises(RuntimeError):
        bq.forward_cpu(dist.double(), 0.2, 4)


def test_bn_momentum_decay_rule_matches_reference():
    """a-13 host logic: the momentum _EpochDecayBatchNorm switches to equals what the reference's MyBatchNorm1d/2d
    end up with (models/layers.py:61-71, :112-121; fixture from the reference itself): no change for epoch None / 0,
    momentum0 * decay ** (epoch // step) from epoch 1 on, clamped below at 0.01, and never reset afterwards."""
    from conftest import load_golden
    from usip_amd.layers import MyBatchNorm1d, MyBatchNorm2d
    g = load_golden("bn_decay_cases.npz")
    for cls in (MyBatchNorm1d, MyBatchNorm2d):
        for e in g["epochs"]:
            epoch = None if e < 0 else int(e)
            bn = cls(4, momentum=0.1, momentum_decay_step=2, momentum_decay=0.6)
            bn.decay_momentum(epoch)
            assert bn.momentum == float(g["momentum_%s" % ("none" if e < 0 else int(e))]), (cls, e)
            assert bn.epoch_driven == (epoch is not None)
        bn = cls(4, momentum=0.1, momentum_decay_step=2, momentum_decay=0.6)
        bn.decay_momentum(9)
        bn.decay_momentum(None)                     # the reference keeps the decayed value
        assert bn.momentum == float(g["momentum_9"])
        bn = cls(4, momentum=0.1, momentum_decay_step=None, momentum_decay=0.6)
        bn.decay_momentum(40)
        assert bn.momentum == 0.1


# ---------------------------------------------------------------------------------------------------------------------
# The shared-MLP GEMM entries refuse what they refused.  Every row below is a call that returns before any launch: a
# well-formed call (the base calls of `_gemm_table`, never issued) with ONE argument broken, or with no positions at all -- the pointers are
# small fake integers, so nothing here may reach a kernel (checked per call through the launch log).
_GEMM_KINDS = {
    "tile": "At lda X X2 coef pro bias rowbias rb_group pool_dp pool_arg pool_group Y y_rows stats M K P nb stream",
    "planes": "planes X X2 coef pro bias rowbias rb_group pool_dp pool_arg pool_group Y y_rows stats M K P nb stream",
    "fork": "planes X X2 coef Y y_rows fork_dp fork_arg fork_group M K P nb stream",
    "red": "planes X X2 coef pro pool_dp pool_arg pool_group Y red_y red_coef red_out red_gsum red_group M K P nb stream",
    "narrow": "At lda X coef pro bias rowbias rb_group Y y_rows stats M K P nb stream",
}
_PTRS = ("At planes X X2 coef bias rowbias pool_dp pool_arg Y stats fork_dp fork_arg red_y red_coef red_out red_gsum").split()
_SET = {p: 0x1000 * (i + 1) for i, p in enumerate(_PTRS)}           # what a present pointer is: 4096-B aligned
_PRO2 = dict(pro=2, X2=_SET["X2"])
_PRO3 = dict(pro=3, X=None, X2=_SET["X2"], pool_dp=_SET["pool_dp"], pool_arg=_SET["pool_arg"], pool_group=4)
_RB = dict(rowbias=_SET["rowbias"])


def _base(kind, **over):
    call = {a: None if a in _PTRS or a == "stream" else 0 for a in _GEMM_KINDS[kind].split()}
    call.update({a: _SET[a] for a in ("At", "planes", "X", "coef", "Y") if a in call})
    call.update(over)
    return call


# entry -> (kind, the well-formed call, what the EMPTY call (P = 0) returns, the broken arguments).  A dict is merged into
# the base; several keys = the prologue that the broken argument belongs to, then the break.
def _gemm_table():
    shared = [dict(pro=0, X=None), dict(X=None), dict(coef=None), dict(_PRO2, X=None), dict(_PRO2, X2=None),
              dict(_PRO2, coef=None), dict(_PRO2, stats=_SET["stats"]), dict(_PRO3, X2=None), dict(_PRO3, coef=None),
              dict(_PRO3, stats=_SET["stats"]), dict(_PRO3, pool_dp=None), dict(_PRO3, pool_arg=None),
              dict(_PRO3, pool_group=0), dict(_PRO3, pool_group=3), dict(_PRO3, pool_group=48),
              dict(_RB, rb_group=0), dict(_RB, rb_group=48), dict(y_rows=63), dict(Y=None), dict(pro=4), dict(pro=-1),
              dict(M=0), dict(K=0), dict(P=-1), dict(nb=-1)]
    tile = _base("tile", lda=64, pro=1, rb_group=1, M=64, K=32, P=64, nb=2)
    tile_own = [dict(At=None), dict(lda=63), dict(lda=-31), dict(_PRO3, pool_group=2)]     # (fp32 entries: pool_group % 4)
    pl = _base("planes", pro=1, rb_group=1, M=64, K=32, P=64, nb=2)
    pl_own = [dict(planes=None), dict(planes=_SET["planes"] + 8), dict(K=641), dict(_PRO2, K=513), dict(_PRO3, K=513)]
    x2r_own = [dict(pro=0), dict(M=129, y_rows=0), dict(K=129), dict(_RB, rb_group=16), dict(_PRO2, **_RB, rb_group=32),
               dict(K=128, P=1 << 23)]
    big = dict(M=256, K=128, P=32768, nb=1)                          # the smallest launch of whole 256 x 256 tiles
    fork = _base("fork", X2=_SET["X2"], fork_dp=_SET["fork_dp"], fork_arg=_SET["fork_arg"], fork_group=16, **big)
    fork_bad = [{p: None} for p in "planes X X2 coef Y fork_dp fork_arg".split()] + [
        dict(planes=_SET["planes"] + 8), dict(M=0), dict(K=0), dict(K=576), dict(nb=0), dict(fork_group=0), dict(fork_group=48),
        dict(fork_group=8), dict(fork_group=128), dict(y_rows=255), dict(M=128), dict(M=300), dict(P=32768 - 256), dict(P=32768 + 128),
        dict(K=160), dict(Y=_SET["Y"] + 4), dict(X=_SET["X"] + 4), dict(X2=_SET["X2"] + 4), dict(fork_dp=_SET["fork_dp"] + 8),
        dict(fork_arg=_SET["fork_arg"] + 8)]
    red = _base("red", pro=2, X2=_SET["X2"], red_y=_SET["red_y"], red_coef=_SET["red_coef"], red_out=_SET["red_out"], **big)
    red3 = dict(pro=3, X=None, pool_dp=_SET["pool_dp"], pool_arg=_SET["pool_arg"], pool_group=16)
    red_bad = [{p: None} for p in "planes X X2 coef Y red_y red_coef red_out".split()] + [
        dict(planes=_SET["planes"] + 8), dict(pro=0), dict(pro=1), dict(pro=4), dict(M=128), dict(M=300), dict(K=0), dict(K=513),
        dict(P=32768 - 128), dict(P=32768 + 64), dict(nb=0), dict(red_gsum=_SET["red_gsum"], red_group=8),
        dict(Y=_SET["Y"] + 4), dict(red_y=_SET["red_y"] + 4), dict(red3, pool_dp=None), dict(red3, pool_arg=None),
        dict(red3, pool_group=0), dict(red3, pool_group=3)]
    nf = _base("narrow", lda=64, pro=1, rb_group=1, M=64, K=64, P=196608, nb=1)
    nf_bad = [dict(At=None), dict(X=None), dict(Y=None), dict(coef=None), dict(lda=63), dict(pro=2), dict(pro=-1), dict(K=32),
              dict(M=32), dict(P=196610), dict(P=196608 - 64), dict(nb=0), dict(X=_SET["X"] + 8), dict(_RB, rb_group=0),
              dict(_RB, rb_group=16), dict(_RB, rb_group=48), dict(_RB, rb_group=160), dict(y_rows=63), dict(y_rows=21846)]
    no_x2h = [dict(pro=0)]                                           # x2h and x2r take prologues 1, 2, 3 only
    table = {"usip_mlp_gemm_%s" % m: ("tile", tile, 0, shared + tile_own) for m in ("f32", "bf16", "f32x3")}
    table["usip_mlp_gemm_x3p_f32"] = ("planes", pl, 0, shared + pl_own)
    table["usip_mlp_gemm_x2h_f32"] = ("planes", pl, 0, shared[1:] + pl_own + no_x2h)
    table["usip_mlp_gemm_x2r_f32"] = ("planes", pl, 0, shared[1:] + pl_own[:2] + x2r_own)
    table["usip_mlp_gemm_x2h_fork_f32"] = ("fork", fork, -1, fork_bad)   # (no empty launch: P, nb >= 1)
    table["usip_mlp_gemm_x2h_red_f32"] = ("red", red, -1, red_bad)       # (the same)
    table["usip_mlp_narrow_forward_f32"] = ("narrow", nf, -1, nf_bad)    # (the same: the shape is not its own)
    return table


def _gemm_rows():
    rows = []
    for entry, (kind, base, empty, bad) in _gemm_table().items():
        assert 16 <= len(bad), entry
        for change in bad:
            call = dict(base, **change)
            assert call != base and (call["P"] != 0), (entry, change)         # never the well-formed call itself
            rows.append((entry, kind, call, -1))
        rows.append((entry, kind, dict(base, P=0), empty))
    return rows


def test_gemm_entries_refuse_what_they_refused():
    from usip_amd import _lib
    lib = _lib.lib()
    assert all(lib.usip_tuning_value(knob) == 0 for knob in range(8))     # the fork and `red` routes read the knobs
    wrong = []
    for entry, kind, call, want in _gemm_rows():
        lib.usip_launch_log(1)
        got = getattr(lib, entry)(*[call[a] for a in _GEMM_KINDS[kind].split()])
        launched = lib.usip_launch_log(0)
        assert launched == 0, (entry, call)
        if got != want:
            wrong.append((entry, {k: v for k, v in call.items() if v}, got, want))
    assert not wrong, wrong


def test_fork_and_red_queries_answer_as_before():
    """usip_mlp_gemm_x2h_fork_supported(M, K, P, nb, fork_group) and usip_mlp_gemm_x2d_red_tiles(M, K, P, nb, red_group) on
    both sides of their thresholds (host arithmetic only); the values are the library's before the GEMM entries shared
    their checks."""
    from usip_amd import _lib
    lib = _lib.lib()
    fork = {(256, 128, 32768, 1, 16): 1, (256, 128, 32512, 1, 16): 0, (512, 128, 16384, 1, 16): 1, (512, 128, 16128, 1, 16): 0,
            (256, 128, 8192, 4, 16): 1, (256, 128, 32768, 1, 8): 0, (256, 128, 32768, 1, 32): 1, (256, 128, 32768, 1, 64): 1,
            (256, 128, 32768, 1, 128): 0, (256, 192, 32768, 1, 16): 1, (256, 160, 32768, 1, 16): 0, (256, 512, 32768, 1, 16): 1,
            (256, 576, 32768, 1, 16): 0, (256, 128, 32896, 1, 16): 0, (300, 128, 32768, 1, 16): 0, (128, 128, 32768, 1, 16): 0,
            (256, 128, 32768, 1, 0): 0, (256, 128, 0, 1, 16): 0}
    red = {(256, 128, 32768, 1, 0): 256, (256, 128, 32768, 1, 16): 256, (256, 128, 32768, 1, 32): 256, (256, 128, 32768, 1, 8): 0,
           (256, 128, 32640, 1, 0): 0, (512, 128, 16384, 1, 0): 128, (512, 128, 16256, 1, 0): 0, (256, 128, 8192, 4, 16): 256,
           (256, 512, 32768, 1, 0): 256, (256, 513, 32768, 1, 0): 0, (256, 16, 32768, 1, 0): 256, (300, 128, 32768, 1, 0): 0,
           (128, 128, 32768, 1, 0): 0, (256, 128, 32832, 1, 0): 0, (256, 128, 32768, 0, 0): 0}
    assert {k: lib.usip_mlp_gemm_x2h_fork_supported(*k) for k in fork} == fork
    assert {k: lib.usip_mlp_gemm_x2d_red_tiles(*k) for k in red} == red
