"""Every form of the shared-MLP GEMM family, bit for bit (csrc/shared_mlp.hip, shared_mlp_bf16.hip, shared_mlp_x3.hip,
gemm_x2d.hip, gemm_x2f.hip, narrow_fwd.hip).

The operands come from tests/gemm_oracle.py: every element is reproduced exactly by the planes its form keeps, every dropped
plane pair has a zero factor, every sum stays below 2^24 units -- so the fp64 product is an fp32 number and independent of
the accumulation order, and each form must EQUAL it: outputs, statistics partials per slot, the fork add.  No tolerance
appears in this file.  tests/test_gemm_oracle_cpu.py asserts the fixtures' claims on the CPU.

Each case names the kernel instantiation it targets (gemm_cases.GEMM_CASES, following tests/golden/gemm_routes_parent.json),
reaches it through ops.mlp_gemm with the existing switches, and asserts from the library's launch log that this
instantiation ran with the expected workgroup count."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_cases as gc
import gemm_oracle as go
from gemm_gpu_helpers import DEV, _Switches, _dev, _logged, _ran

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [n for n, c in gc.GEMM_CASES.items() if not c["opt"].get("c_entry")])
def test_gemm_form_equals_the_exact_product(name):
    from usip_amd import _lib, ops
    lib = _lib.lib()
    c = gc.GEMM_CASES[name]
    o = c["opt"]
    fx = gc.case_fixture(name)
    nb, K, M, P, pro = c["nb"], c["K"], c["M"], c["P"], c["pro"]
    a_trans, a_off = bool(o.get("a_trans")), int(o.get("a_offset", 0))
    lda = (K if a_trans else M) + (a_off + 2 if a_off else 0)
    At = _dev(go.at_storage(fx["A"], lda, a_off, a_trans))
    X, X2, coef = _dev(fx["X"]), _dev(fx["X2"]), _dev(fx["coef"])
    kw = dict(bias=_dev(fx["bias"]), want_stats=fx["stats"] is not None, pro=pro, X2=X2, coef=coef, a_trans=a_trans,
              a_offset=a_off, M=M, tag="fwd" if pro < 2 else "dgrad")
    if fx["rowbias"] is not None:
        kw.update(rowbias=_dev(fx["rowbias"]), rb_group=fx["rb_group"])
    if pro == 3:
        dp, arg, g = fx["pool"]
        kw["pool"] = (_dev(dp), _dev(arg), g)
    if o.get("fork"):
        fdp, farg, fg = fx["fork"]
        kw["fork"] = (_dev(fdp), _dev(farg), fg)
    if "red" in fx:
        kw.update(red=(_dev(fx["red"]["y"]), _dev(fx["red"]["coef"])), red_group=o["red"])
    wide = None
    if o.get("wider"):                                         # rows [3, 3 + M) of a wider tensor; P % 4 != 0 leaves Y unaligned
        wide = torch.full((nb, M + 5, P), float("nan"), device=DEV)
        kw.update(out=wide, out_row_offset=3)
    with _Switches(c["mode"], o.get("knobs"), o.get("cache", False), fold=True):      # (POOL_GRAD_FOLD on: the fork cases' route)
        if pro == 1:
            ops.declare_samples(coef, nb * P)                  # hand-built statistics: taken over this launch's samples
        res, got = _logged(lib, lambda: ops.mlp_gemm(At, X, **kw))
        if o.get("cache"):                                     # a second call finds the image in the cache: the same bits
            res2, got2 = _logged(lib, lambda: ops.mlp_gemm(At, X, **kw))
            assert not any("split3" in n for n, _ in got2), got2
            assert torch.equal(res2[0], res[0])
        torch.cuda.synchronize()
    _ran(got, c["kernel"], c["wgs"])
    Y = res[0] if wide is None else wide[:, 3:3 + M]
    want = _dev(fx["want"])
    assert Y.shape == want.shape
    assert torch.equal(Y, want), "%d of %d outputs differ" % (int((Y != want).sum()), want.numel())
    if wide is not None:
        assert bool(torch.isnan(wide[:, :3]).all()) and bool(torch.isnan(wide[:, 3 + M:]).all())
    if fx["stats"] is not None:
        st = _dev(fx["stats"])
        assert res[1].shape == st.shape, (res[1].shape, st.shape)
        assert torch.equal(res[1], st), "%d of %d statistics partials differ" % (int((res[1] != st).sum()), st.numel())
    if o.get("fork"):
        assert res[2] is True
    if "red" in fx:                                            # sums and maxima per tile, the per-run sums, and what carries them
        r = fx["red"]
        assert isinstance(res[2], ops.RedSums)
        assert torch.equal(res[2].sums, _dev(r["sums"])) and torch.equal(res[2].maxima, _dev(r["maxima"]))
        assert (res[2].gsum is None) == (r["gsum"] is None)
        if r["gsum"] is not None:
            assert torch.equal(res[2].gsum, _dev(r["gsum"]))


def test_register_resident_gemm_at_64_rows_through_the_c_entry():
    """gemm_x2r_kernel with half its rows: usip_mlp_gemm_x2r_f32 on the two-plane image ops.weight_planes hands out"""
    from usip_amd import _lib, ops
    lib = _lib.lib()
    name = "x2r M64 through the C entry"
    c, fx = gc.GEMM_CASES[name], gc.case_fixture(name)
    nb, K, M, P = c["nb"], c["K"], c["M"], c["P"]
    At, X, coef, bias = _dev(go.at_storage(fx["A"], M, 0)), _dev(fx["X"]), _dev(fx["coef"]), _dev(fx["bias"])
    planes = ops.weight_planes(At, 0, M, K, 2, P, nb)
    Y = torch.full((nb, M, P), float("nan"), device=DEV)
    stats = torch.full((2, M, int(lib.usip_mlp_gemm_x2r_tiles(P, nb))), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc, got = _logged(lib, lambda: lib.usip_mlp_gemm_x2r_f32(p(planes), p(X), None, p(coef), 1, p(bias), None, 1, None, None, 0,
                                                             p(Y), 0, p(stats), M, K, P, nb, st))
    assert rc == 0
    torch.cuda.synchronize()
    _ran(got, c["kernel"], c["wgs"])
    assert torch.equal(Y, _dev(fx["want"])) and stats.shape == fx["stats"].shape and torch.equal(stats, _dev(fx["stats"]))


# ------------------------------------------------------------------------------------------------ weight images
def _operand(kind, M, K, rng):
    A = go.exact32(rng.integers(-9000, 9001, (M, K)) * 2.0 ** -9, "A")
    if kind == "zero":
        A[:] = 0.0
    elif kind == "pow2":                                       # the maximum is a power of two
        A = np.clip(A, -7.5, 7.5)
        A.reshape(-1)[(M * K) // 2] = -8.0
    elif kind == "below":                                      # ... and just below one
        A = np.clip(A, -7.5, 7.5)
        A.reshape(-1)[0] = np.float32(8.0 - 2.0 ** -20)
    return A


IMAGE_CASES = [(1, 1, 128, "rand"), (1, 1, 256, "rand"), (128, 16, 128, "rand"), (128, 17, 256, "pow2"), (129, 17, 128, "below"),
               (129, 16, 256, "rand"), (300, 17, 128, "pow2"), (300, 16, 256, "below"), (129, 1, 256, "zero"), (40, 33, 128, "zero")]


@pytest.mark.parametrize("M,K,bm,kind", IMAGE_CASES)
@pytest.mark.parametrize("form", ["x3", "x2h"])
def test_split_weight_image(form, M, K, bm, kind):
    """usip_mlp_split3_f32 / usip_mlp_split2h_f32 through the C entry: planes, half swap, stage order, zero padding beyond
    M x K, the scale in trailer float 0 and nothing written behind the trailer -- with a_offset and lda > M.  An all-zero
    operand yields an all-zero image and the scale 2^60."""
    from usip_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(M * 100 + K + bm)
    A = _operand(kind, M, K, rng)
    a_off, lda = 3, M + 7
    At = _dev(go.at_storage(A, lda, a_off, fill=1e9))          # (a neighbour that is read would wreck the scale)
    npl = go.NPLANES[form]
    nbytes = go.image_bytes(M, K, bm, npl)
    buf = torch.full((nbytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
    fn = lib.usip_mlp_split3_f32 if form == "x3" else lib.usip_mlp_split2h_f32
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    (rc, got) = _logged(lib, lambda: fn(ctypes.c_void_p(At.data_ptr() + 4 * a_off), lda, M, K, bm, ctypes.c_void_p(buf.data_ptr()), st))
    assert rc == 0
    torch.cuda.synchronize()
    _ran(got, "split3_tiles_kernel", ((M + bm - 1) // bm) * ((K + 15) // 16))
    want, scale = go.image_ref(A, bm, form)
    img = buf[:nbytes].cpu().numpy().view(np.uint16)
    assert np.array_equal(img, want), "%d of %d image halfwords differ" % (int((img != want).sum()), want.size)
    tail = buf[nbytes:].cpu().numpy()
    if form == "x3":
        assert np.all(tail == 0xA5)
    else:
        tr = tail[:4 * (4 + go.X2H_PARTS)].view(np.float32)
        assert float(tr[0]) == float(scale) and np.all(tail[4:16] == 0xA5) and np.all(tail[4 * (4 + go.X2H_PARTS):] == 0xA5)
        assert float(tr[4:].max()) == float(np.abs(A).max())   # the partial maxima combine to max |A|
        if kind == "zero":
            assert float(scale) == 2.0 ** 60 and not img.any()


def test_multi_operand_split_equals_the_single_one():
    """usip_mlp_split3_multi_f32 (PlanesPlan.refresh) writes, for every operand of a step, the image the single-operand entry
    writes: byte for byte over the image and trailer float 0 -- three- and two-plane operands, both tile row sizes, column
    offsets inside one parameter storage."""
    from usip_amd import _lib, ops
    lib = _lib.lib()
    rng = np.random.default_rng(11)
    K, lda = 40, 700
    store = np.zeros((K, lda), np.float32)
    specs = [(0, 129, 3, 200, 1), (129, 128, 2, 200, 1), (257, 300, 2, 32768, 1), (257, 300, 3, 512, 1), (560, 100, 2, 64, 2)]
    for off, M, _, _, _ in specs:
        store[:, off:off + M] = _operand("rand", M, K, rng).T
    At = _dev(store)
    prev = ops.PLANES_CACHE
    ops.PLANES_CACHE = {}
    try:
        single = []
        for off, M, npl, P, nb in specs:
            pl = ops.weight_planes(At, off, M, K, npl, P, nb)
            rows = int(lib.usip_mlp_x3p_tile_rows(M, P, nb))
            n = go.image_bytes(M, K, rows, npl) + (4 if npl == 2 else 0)
            want, scale = go.image_ref(store[:, off:off + M].T, rows, "x2h" if npl == 2 else "x3")
            got = pl[:n].cpu().numpy()
            assert np.array_equal(got[:want.size * 2].view(np.uint16), want)
            if npl == 2:
                assert float(got[-4:].view(np.float32)[0]) == float(scale)
            single.append((pl, n, got.copy()))
        assert {lib.usip_mlp_x3p_tile_rows(M, P, nb) for _, M, _, P, nb in specs} == {128, 256}
        plan = ops.PlanesPlan(ops.PLANES_CACHE, [At])
        assert len(plan.entries) == len(specs)
        for pl, _, _ in single:
            pl.zero_()
        (fresh, got) = _logged(lib, plan.refresh)
        torch.cuda.synchronize()
        _ran(got, "split3_multi_kernel", plan.blocks)
        for pl, n, ref in single:
            assert np.array_equal(pl[:n].cpu().numpy(), ref)
    finally:
        ops.PLANES_CACHE = prev


def test_which_entries_accept_an_empty_call():
    """Contracts pinned on the way: a call without positions returns USIP_OK from usip_mlp_gemm_f32,
    usip_mlp_gemm_x3p_f32 (whatever its prologue), usip_mlp_gemm_x2h_f32 and usip_mlp_gemm_x2r_f32 before any pointer is looked
    at; the two-plane entries still refuse pro 0 (an unbounded operand has no scale), usip_mlp_gemm_x2r_f32 still checks its
    row-bias rule, and the fork entry takes no empty launch.  usip_mlp_split3_multi_f32 with no operand is a no-op."""
    from usip_amd import _lib
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    some = torch.zeros(64, device=DEV)
    ptr = ctypes.c_void_p(some.data_ptr())
    M, K = 128, 32

    def tail(pro, rowbias=None, rb_group=1, P=0, nb=1):
        return (None, None, None, pro, None, rowbias, rb_group, None, None, 0, None, 0, None, M, K, P, nb, st)
    assert lib.usip_mlp_gemm_f32(None, M, *tail(0)) == 0
    assert lib.usip_mlp_gemm_f32(None, M, *tail(0, P=64, nb=0)) == 0
    assert lib.usip_mlp_gemm_x3p_f32(None, *tail(0)) == 0 and lib.usip_mlp_gemm_x3p_f32(None, *tail(7)) == 0
    assert lib.usip_mlp_gemm_x3p_f32(None, *tail(0, P=64)) != 0                 # positions and no planes
    assert lib.usip_mlp_gemm_x2h_f32(None, *tail(1)) == 0 and lib.usip_mlp_gemm_x2h_f32(None, *tail(3)) == 0
    assert lib.usip_mlp_gemm_x2h_f32(None, *tail(0)) != 0
    assert lib.usip_mlp_gemm_x2r_f32(None, *tail(1)) == 0 and lib.usip_mlp_gemm_x2r_f32(None, *tail(0)) != 0
    assert lib.usip_mlp_gemm_x2r_f32(None, *tail(1, ptr, 32)) == 0
    assert lib.usip_mlp_gemm_x2r_f32(None, *tail(1, ptr, 16)) != 0 and lib.usip_mlp_gemm_x2r_f32(None, *tail(2, ptr, 32)) != 0
    assert lib.usip_mlp_gemm_x2h_fork_f32(ptr, ptr, ptr, ptr, ptr, 0, ptr, ptr, 16, 256, 64, 0, 1, st) != 0
    assert lib.usip_mlp_gemm_x2h_fork_supported(256, 64, 0, 1, 16) == 0
    assert lib.usip_mlp_split3_multi_f32(None, 0, 0, st) == 0
    torch.cuda.synchronize()
