"""The reduce-by-destination kernels (csrc/segment.hip, csrc/knn_layer.hip, the values side of csrc/index_max.hip) against
tests/segment_oracle.py on every dispatch path.  Bit for bit wherever the oracle asserts exactness or follows the kernel's
order; a bound counted in roundings, written next to the case, where it does neither.  Every case asserts from the library's
launch log which kernel ran.

Which case reaches which kernel:
  csr_build_kernel                      P = 0, 1, 63..65, 511..513 (wave slices of 64: one wave, all eight, ragged), 4097 (the
                                        second 8 x 64 trip of wave 0), 16384; N = 1, 2, 513, 1025, 1537, 1820 (scan slots 1..4)
  segment_sum_kernel<1, true>           small B C: `1t`, `coff`, `lengths`, `n513`, `n1820`; P = 8196 and 16384 at B C/2 = 512
  segment_sum_kernel<1, false>          `1f_p` (P % 4 = 3), `1f_view` (src 4 bytes into a larger buffer)
  segment_sum_kernel<2, true>           `2t` (B = 256, C = 3, P = 8: odd C, the last workgroup has one real row), P = 8192
  segment_sum_kernel<2, false>          `2f` (the same with P = 7)
  knn_layer_fwd_kernel                  every segment_oracle.KNN_CASES entry; want_stats=False; ldw = 9 through the C entry
  knn_layer_bwd_kernel<2, 512>          even Cout and P <= 8192, relu 0 and 1; destinations past NT: n513 (one), n1489 (977);
                                        the prefetch hand-over: `handover`, `one_list`; chunk loop: chunk2048 / 4096 / 8320
  knn_layer_bwd_kernel<1, 256>          by itself: odd Cout (cout1, handover_odd, cout9, cout7_p1028, p16384_odd) and
                                        P > 8192 (p8196, p16384); by knob r5_forms = 128 for every two-row case (equal dU bits);
                                        p4100 ends inside the second 256 x 4 x 4 trip; n513: 257 destinations past NT
  index_max_kernel<1, *, true, 256>     ch1, ch1_ctot, k257, k4096, k8192, n4, n1024, n1028
  index_max_kernel<1, 1, false, 256>    n1, n3, n1023 (N % 4 != 0); ch1 with index 4 bytes into a larger buffer
  index_max_kernel<2 | 4 | 8, ...>      ch2 by shape; ch2 with knob index_max_ch = 4; c8 with knob 4 and 8
  index_max_values_bwd_dense_kernel<true | false>   N % 4 == 0 and aligned | the others; with and without src, soff = 1
  index_max_values_bwd_add_kernel       every node-max case, coff = 1 inside C + 2 channels"""
import ctypes

import numpy as np
import pytest
import torch

import segment_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _off4(a):
    """the same values in a contiguous view that starts 4 bytes into a larger buffer: not 16-byte aligned"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return so.bits(_np(t))


def _launched(call):
    """-> (call(), [(kernel, workgroups)] of the launches the library made for it, names without namespace and arguments)"""
    from usip_amd import _lib
    lib = _lib.lib()
    lib.usip_launch_log(1)
    try:
        out, got, wg = call(), [], ctypes.c_uint()
        while (name := lib.usip_launch_log_entry(len(got), ctypes.byref(wg))) is not None:
            short = name.decode().replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            got.append((short, int(wg.value)))
    finally:
        lib.usip_launch_log(0)
    return out, got


class _knob:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from usip_amd import _lib
        assert _lib.lib().usip_set_tuning(self.name, self.value) == 0

    def __exit__(self, *exc):
        from usip_amd import _lib
        _lib.lib().usip_set_tuning(self.name, 0)


# ----------------------------------------------------------------------------------------------- csr_by_index
def _csr(idx, N):
    from usip_amd import ops
    (start, perm), log = _launched(lambda: ops.csr_by_index(_dev(idx), N))
    assert log == ([("csr_build_kernel", idx.shape[0])] if idx.shape[0] else []), log
    return _np(start), _np(perm)


def _random_idx(seed, B, P, N, junk=True):
    """cells 0 and N - 1 stay empty (N >= 3); every 17th entry is out of range, negative and >= N in turn"""
    rng = np.random.default_rng(seed)
    lo, hi = (1, N - 1) if N >= 3 else (0, N)
    idx = rng.integers(lo, hi, (B, P)).astype(np.int32)
    if junk:
        idx[:, 5::34], idx[:, 22::34] = -1, N
    return idx


@pytest.mark.parametrize("P", (0, 1, 63, 64, 65, 511, 512, 513, 4097, 16384))
def test_csr_every_cell_of_every_cloud(P):
    B, N = 3, 40
    idx = _random_idx(P, B, P, N)
    start, perm = _csr(idx, N)
    so.check_perm(idx, N, start, perm)
    assert (start[:, 1] == 0).all() and (start[:, N] == start[:, N - 1]).all()      # cells 0 and N - 1 are empty
    start2, perm2 = _csr(idx, N)
    assert np.array_equal(start, start2) and np.array_equal(perm, perm2)              # the same segments on every launch


@pytest.mark.parametrize("N", (1, 2, 513, 1025, 1537, 1820))
def test_csr_every_scan_slot(N):
    B, P = 2, 2500
    idx = _random_idx(N, B, P, N)
    start, perm = _csr(idx, N)
    so.check_perm(idx, N, start, perm)
    assert so.segment_claims(idx, N)["junk"] >= 100


def test_csr_one_cell_holds_everything_and_no_cloud_is_no_launch():
    from usip_amd import ops
    P, N = 4097, 7
    idx = np.full((2, P), 5, np.int32)
    start, perm = _csr(idx, N)
    so.check_perm(idx, N, start, perm)
    assert np.array_equal(np.sort(perm, axis=1), np.broadcast_to(np.arange(P), (2, P)))
    start, perm = _csr(np.zeros((0, 16), np.int32), N)
    assert start.shape == (0, N + 1) and perm.shape == (0, 16)
    for refused in (1821, 2049):
        with pytest.raises(RuntimeError):
            ops.csr_by_index(_dev(np.zeros((1, 16), np.int32)), refused)


# ----------------------------------------------------------------------------------------------- segment_sum
# name -> (B, C, channels in front, channels behind, N, P, lengths of the first cells or None, src offset, kernel, workgroups)
SEGMENT_CASES = {
    "1t": (2, 3, 0, 0, 40, 512, None, False, "segment_sum_kernel<1, true>", 6),
    "coff": (2, 3, 2, 1, 40, 512, None, False, "segment_sum_kernel<1, true>", 6),
    "lengths": (2, 2, 0, 0, 9, 64, (0, 1, 3, 4, 5, 7, 8), False, "segment_sum_kernel<1, true>", 4),
    "one_cell": (2, 2, 0, 0, 3, 516, (0, 516), False, "segment_sum_kernel<1, true>", 4),
    "1f_p": (2, 3, 1, 0, 40, 515, None, False, "segment_sum_kernel<1, false>", 6),
    "1f_view": (2, 3, 0, 0, 40, 512, None, True, "segment_sum_kernel<1, false>", 6),
    "2t": (256, 3, 0, 0, 4, 8, None, False, "segment_sum_kernel<2, true>", 512),
    "2f": (256, 3, 0, 1, 4, 7, None, False, "segment_sum_kernel<2, false>", 512),
    "n513": (2, 3, 0, 0, 513, 4096, None, False, "segment_sum_kernel<1, true>", 6),
    "n1820": (2, 3, 0, 0, 1820, 4096, None, False, "segment_sum_kernel<1, true>", 6),
    # B ceil(C / 2) = 512: two rows while they fit 64 KiB, then one
    "p8192": (2, 512, 0, 0, 64, 8192, None, False, "segment_sum_kernel<2, true>", 512),
    "p8196": (2, 512, 0, 0, 64, 8196, None, False, "segment_sum_kernel<1, true>", 1024),
    "p16384": (2, 512, 0, 0, 64, 16384, None, False, "segment_sum_kernel<1, true>", 1024),
}


@pytest.mark.parametrize("name", sorted(SEGMENT_CASES))
def test_segment_sum_is_the_float32_chain_in_list_order(name):
    """random normal data: the kernel's order is fixed and known from perm, so the sums are held to bit patterns"""
    from usip_amd import ops
    B, C, pre, post, N, P, lengths, off, kernel, wgs = SEGMENT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    idx = _random_idx(P + N, B, P, N) if lengths is None else np.stack([so.idx_of_lengths(rng, lengths, N, P) for _ in range(B)])
    if lengths is not None:
        assert set(lengths) <= so.segment_claims(idx, N)["lengths"]
    start, perm = _csr(idx, N)
    so.check_perm(idx, N, start, perm)
    src = np.full((B, pre + C + post, P), np.nan, np.float32)                # NaN in every channel outside the slice
    src[:, pre:pre + C] = rng.standard_normal((B, C, P), dtype=np.float32)
    s = _off4(src) if off else _dev(src)
    assert ops.segment_sum_supported(N, P)
    dx, log = _launched(lambda: ops.segment_sum(s, _dev(start), _dev(perm), C, pre))
    assert log == [(kernel, wgs)], log
    want = so.segment_sum_listorder(src, start, perm, C, pre)
    assert np.array_equal(_bits(dx), so.bits(want))
    ref = so.segment_sum64(src, idx, C, N, pre)                              # and the list order sums the right members
    assert np.abs(want - ref).max() <= 2.0 ** -24 * (so.segment_claims(idx, N)["longest"] + 2) * np.abs(src[:, pre:pre + C]).sum(axis=2).max()


def test_segment_sum_refuses_a_row_beyond_the_lds():
    from usip_amd import ops
    assert ops.segment_sum_supported(64, 16384) and not ops.segment_sum_supported(64, 16388)
    idx = np.zeros((1, 16388), np.int32)
    start, perm = _csr(idx, 4)
    with pytest.raises(RuntimeError):
        ops.segment_sum(torch.zeros(1, 1, 16388, device=DEV), _dev(start), _dev(perm), 1)


# ----------------------------------------------------------------------------------------------- KNN first layer, forward
def _knn_forward(c, **kw):
    from usip_amd import ops
    return ops.knn_layer_forward(_dev(c["U"]), _dev(c["W"]), _dev(c["database"]), _dev(c["query"]), _dev(c["idx"]), **kw)


@pytest.mark.parametrize("name", sorted(so.KNN_CASES))
def test_knn_layer_forward_bits_and_statistics(name):
    from usip_amd import ops
    c = so.knn_case(name)
    assert so.knn_claims_hold(name, c["claims"]), c["claims"]
    B, Cout, N = c["U"].shape
    _, M, K = c["idx"].shape
    P = M * K
    assert ops.knn_layer_supported(N, M, K)
    (Y, stats), log = _launched(lambda: _knn_forward(c))
    assert log == [("knn_layer_fwd_kernel", -(-Cout // 8) * B)], log
    want, _, _ = so.knn_forward(c["U"], c["W"], c["database"], c["query"], c["idx"])
    assert np.array_equal(_bits(Y), so.bits(want))
    terms = so.knn_stats(want)                                              # [2][Cout][B] partials: one per cloud
    got = _np(stats).reshape(2, Cout, B)
    # the longest chain of additions: 4 per trip of 4 x 256 positions and thread, 6 shuffle steps, 2 levels over the four waves
    chain = 4 * -(-P // 1024) + 6 + 2
    for s, step in ((0, 4), (1, 8)):
        ref = terms[s].sum(axis=-1)
        ok = so.any_order_exact(terms[s], step)
        assert np.array_equal(so.bits(got[s][ok]), so.bits(ref[ok].astype(np.float32))), (name, s)
        err, bound = np.abs(got[s].astype(np.float64) - ref), so.rounding_bound(terms[s], chain)
        print(name, "sum" if s == 0 else "sum^2", "exact partials:", int(ok.sum()), "of", ok.size,
              "worst error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, s)
    (Y2, none), log = _launched(lambda: _knn_forward(c, want_stats=False))
    assert none is None and log == [("knn_layer_fwd_kernel", -(-Cout // 8) * B)] and torch.equal(Y, Y2)


def test_knn_layer_forward_reads_a_weight_with_a_longer_row_stride():
    """ldw = 9 over rows of 5: the wrapper asks for a contiguous weight, so this goes through the C entry"""
    from usip_amd import _lib, ops
    c = so.knn_case("cout9")
    B, Cout, N = c["U"].shape
    _, M, K = c["idx"].shape
    wide = torch.full((Cout, 9), float("nan"), device=DEV)
    wide[:, :5] = _dev(c["W"])
    W = wide[:, :5]
    assert W.stride(0) == 9 and not W.is_contiguous()
    t = [_dev(c[k]) for k in ("U", "database", "query", "idx")]
    Y = torch.empty((B, Cout, M * K), device=DEV)
    p = [ctypes.c_void_p(x.data_ptr()) for x in t]
    rc = _lib.lib().usip_knn_layer_forward_f32(p[0], ctypes.c_void_p(W.data_ptr()), 9, p[1], p[2], p[3],
                                               ctypes.c_void_p(Y.data_ptr()), None, B, Cout, N, M, K,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert np.array_equal(_bits(Y), so.bits(so.knn_forward(c["U"], c["W"], c["database"], c["query"], c["idx"])[0]))
    assert not ops.knn_layer_supported(1490, 8, 4) and ops.knn_layer_supported(1489, 8, 4)


# ----------------------------------------------------------------------------------------------- KNN first layer, backward
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("name", sorted(so.KNN_CASES))
def test_knn_layer_backward_bits_in_both_forms(name, relu):
    from usip_amd import ops
    c = so.knn_case(name)
    B, Cout, N = c["U"].shape
    _, M, K = c["idx"].shape
    P = M * K
    idx = np.clip(c["idx"].reshape(B, P), 0, N - 1)
    start, perm = _csr(idx, N)
    so.check_perm(idx, N, start, perm)
    _, d, _ = so.knn_forward(c["U"], c["W"], c["database"], c["query"], c["idx"])
    g = so.knn_backward_g(c["dZ"], c["Yb"], c["coef4"], relu)
    if name in ("handover", "cout9"):                                       # the flag changes something
        assert not np.array_equal(g, so.knn_backward_g(c["dZ"], c["Yb"], c["coef4"], not relu))
    want_dU = so.segment_sum_listorder(g, start, perm, Cout)
    terms = so.knn_dwc_terms(g, d)                                          # [Cout, 3, B P]
    args = (_dev(c["dZ"]), _dev(c["Yb"]), _dev(c["coef4"]), relu, _dev(d), _dev(start), _dev(perm), M, K)
    two = Cout % 2 == 0 and P <= 8192
    tpw = 1
    while tpw < 8 and (B * Cout // 2) // (tpw * 2) >= 2 * _cus():          # knn_layer.hip: chunks per workgroup
        tpw *= 2
    forms = [(0, "knn_layer_bwd_kernel<2, 512>", 512, B * -(-(Cout // 2) // tpw))] if two else []
    forms.append((128, "knn_layer_bwd_kernel<1, 256>", 256, B * -(-Cout // tpw)))
    if name in so.CHUNK_TPW:
        print(name, "compute units:", _cus(), "chunks per workgroup:", tpw, "workgroups:", forms[0][3])
        if _cus() == 256:
            assert tpw == so.CHUNK_TPW[name] and forms[0][3] == B * -(-(Cout // 2) // so.CHUNK_TPW[name])
    for knob, kernel, NT, wgs in forms:
        with _knob(b"r5_forms", knob if two else 0):                        # the one-row form by itself where two rows cannot run
            (dU, dwc), log = _launched(lambda: ops.knn_layer_backward(*args))
        assert log == [(kernel, wgs)], (log, kernel, wgs)
        assert np.array_equal(_bits(dU), so.bits(want_dU)), (name, kernel)   # every channel, every destination
        # dWc: 4 fused multiply-adds per 16-byte piece and ceil(P / (4 NT 4)) * 4 pieces per thread at most, 6 shuffle steps,
        # NT / 64 waves in order, B per-cloud partials
        chain = 4 * 4 * -(-P // (16 * NT)) + 6 + NT // 64 + B
        ref = terms.sum(axis=-1)
        ok = so.any_order_exact(terms, 8)
        got = _np(dwc)
        assert np.array_equal(so.bits(got[ok]), so.bits(ref[ok].astype(np.float32))), (name, kernel)
        err, bound = np.abs(got.astype(np.float64) - ref), so.rounding_bound(terms, chain)
        print(name, kernel, "dWc exact:", int(ok.sum()), "of", ok.size, "worst error / bound:",
              float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, kernel)


def test_knn_layer_backward_refuses_a_misaligned_operand():
    """dZ, Y and dcoord are read in 16-byte pieces: the return code, and nothing launched"""
    from usip_amd import _lib
    c = so.knn_case("cout1")
    B, Cout, N = c["U"].shape
    _, M, K = c["idx"].shape
    P = M * K
    start, perm = _csr(np.clip(c["idx"].reshape(B, P), 0, N - 1), N)
    d = np.zeros((B, 3, P), np.float32)
    dU, part = torch.empty((B, Cout, N), device=DEV), torch.empty((B, Cout, 3), device=DEV)
    fixed = [_dev(c["coef4"]), _dev(start), _dev(perm)]
    for bad in range(3):
        t = [(_off4 if i == bad else _dev)(a) for i, a in enumerate((c["dZ"], c["Yb"], d))]
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        rc, log = _launched(lambda: _lib.lib().usip_knn_layer_backward_f32(
            p(t[0]), p(t[1]), p(fixed[0]), 1, p(t[2]), p(fixed[1]), p(fixed[2]), p(dU), p(part), B, Cout, N, M, K,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert rc < 0 and log == [], (bad, rc, log)


# ----------------------------------------------------------------------------------------------- node-max values
def _index_max_kernel(B, C, N, K, aligned=True):
    from usip_amd import ops
    ch, u, t = ops.index_max_geometry(B, C, N, K)
    if N % 4 == 0 and aligned:
        return ch, "index_max_kernel<%d, %d, true, %d>" % (ch, u, t), B * (C // ch)
    return ch, "index_max_kernel<%d, 1, false, 256>" % ch, B * (C // ch)


def _values(c, count=True, index=None, want_ch=None):
    from usip_amd import ops
    data, idx = _dev(c["data"]), _dev(c["index"]) if index is None else index
    B, Ctot, N = c["data"].shape
    ch, kernel, wgs = _index_max_kernel(B, c["C"], N, c["K"], idx.data_ptr() % 16 == 0)
    assert want_ch is None or ch == want_ch, (ch, want_ch)
    cnt = _dev(c["count"]) if count else None
    (mi, val), log = _launched(lambda: ops.index_max_values(data, idx, cnt, c["K"], C=c["C"]))
    assert log == [(kernel, wgs)], (log, kernel)
    want_mi, want_val = so.index_max_values(c["data"], c["index"], c["count"] if count else None, c["K"], c["C"])
    assert np.array_equal(_np(mi), want_mi)
    nan = np.isnan(want_val)                                                # an all-below-floor node reports data[b, c, 0]
    assert np.array_equal(np.isnan(_np(val)), nan) and np.array_equal(_bits(val)[~nan], so.bits(want_val)[~nan])
    return kernel


@pytest.mark.parametrize("name", sorted(so.NODEMAX_CASES))
def test_node_max_values_and_both_backwards(name):
    from usip_amd import ops
    c = so.nodemax_case(name)
    assert so.nodemax_claims_hold(name, c["claims"]), c["claims"]
    B, Ctot, N = c["data"].shape
    C, K = c["C"], c["K"]
    kernel = _values(c, want_ch=2 if name == "ch2" else 1)
    assert ("true" in kernel) == (N % 4 == 0)
    _values(c, count=False)
    mi = so.index_max(c["data"], c["index"], K, C)
    assert mi.min() >= 0 and mi.max() < max(N, 1)
    # the dense backward, without and with a source slice (soff = 1 inside C + 2 channels)
    for src in (None, c["src"]):
        want = so.index_max_scatter(c["g"], mi, c["count"], N, None if src is None else src[:, 1:1 + C])
        dz, log = _launched(lambda: ops.index_max_values_backward(_dev(c["g"]), _dev(mi), _dev(c["count"]), _dev(c["index"]), N,
                                                                  src=None if src is None else _dev(src), soff=1 if src is not None else 0))
        assert log == [("index_max_values_bwd_dense_kernel<%s>" % ("true" if N % 4 == 0 else "false"), B * C)], log
        assert np.array_equal(_bits(dz), so.bits(want)), (name, src is None)
    dz = ops.index_max_values_backward(_dev(c["g"]), _dev(mi), None, _dev(c["index"]), N)       # count=None: every node counts
    assert np.array_equal(_bits(dz), so.bits(so.index_max_scatter(c["g"], mi, None, N)))
    # the scatter-add into a gradient that exists: coff = 1; every other element keeps its bits
    base = np.array(c["src"])
    want = base.copy()
    want[:, 1:1 + C] = so.index_max_scatter(c["g"], mi, c["count"], N, base[:, 1:1 + C])
    dd = _dev(base)
    out, log = _launched(lambda: ops.index_max_values_backward_add_(dd, _dev(c["g"]), _dev(mi), _dev(c["count"]), coff=1))
    assert log == [("index_max_values_bwd_add_kernel", -(-B * C * K // 256))], log
    assert out.data_ptr() == dd.data_ptr() and np.array_equal(_bits(dd), so.bits(want))


def test_node_max_values_scalar_path_by_a_misaligned_index_and_rows_by_knob():
    c = so.nodemax_case("ch1")
    assert "false" in _values(c, index=_off4(c["index"]))
    for name, ch in (("ch2", 4), ("c8", 4), ("c8", 8)):
        with _knob(b"index_max_ch", ch):
            _values(so.nodemax_case(name), want_ch=ch)
            _values(so.nodemax_case(name), count=False, want_ch=ch)


def test_node_max_value_of_a_winning_negative_zero_is_positive_zero():
    """The contract (csrc/index_max.hip): values equal gather * mask numerically; a winning -0.0 comes back as +0.0, where
    the reference's gather carries -0.0.  The index is the first of the zeros of either sign."""
    from usip_amd import ops
    data = np.asarray([[[-1.0, -0.0, 0.0, -2.0, -0.0, -3.0, -0.0, -0.5]]], np.float32)
    index = np.asarray([[0, 0, 0, 0, 1, 1, 2, 3]], np.int32)
    count = np.asarray([[4, 2, 1, 1]], np.int32)
    mi, val = ops.index_max_values(_dev(data), _dev(index), _dev(count), 4)
    want_mi, want_val = so.index_max_values(data, index, count, 4)
    assert want_mi.tolist() == [[[1, 4, 6, 7]]] and np.signbit(want_val[0, 0, :3]).all()
    assert np.array_equal(_np(mi), want_mi)
    assert np.array_equal(_np(val), want_val)                               # numerically: -0.0 == +0.0
    assert not np.signbit(_np(val)[0, 0, :3]).any() and _bits(val)[0, 0, 3] == so.bits(np.float32(-0.5))
