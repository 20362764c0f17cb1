"""The seven kernels of the loss tail (csrc/nearest.hip, csrc/chamfer.hip) on the MI355X at their edges, against the plain
references of tests/loss_oracle.py (which test_loss_oracle_cpu.py anchors to the reference project's fixture).

  ops.nearest             value and first index BIT FOR BIT: random clouds against torch.norm + torch.min, lattice clouds
                          (exact integer squares, ties in nearly every query) against integer arithmetic; every shape at
                          which the launcher or the kernel takes another path (loss_oracle.chunk_plan, held to the library
                          by the CPU test), and hand-placed minima, ties, rings, overflow and NaN.
  ops.nearest_nd          both templates, channel counts that leave a tail of the unrolled channel loop; lattice
                          descriptors bit for bit, unit-norm descriptors within bounds derived from the FMA chain.
  ops.nearest_backward    float64 at the kernel's own decisions, within bounds counted in roundings; staging chunks,
                          quarter splits, channel-slice tails, a partner of everybody and partners of nobody.
  ops.chamfer_prob(+bwd)  float64 autograd, bounds counted in roundings against sums of MAGNITUDES.
  losses.*                the autograd wiring of the two modules built on them.

Every derived bound prints its worst err / bound (run with -s to see them).  The worst over all cases, measured on one
MI355X: nearest_nd value 0.48, index 0.00; nearest_backward ga 0.36, gb 0.18; chamfer loss 0.17 (sigmas at 1e-3; 0.08
otherwise), pure 0.25, weighted 0.16, da 0.71, dc 0.80, dss 0.46, dsd 0.45.  No bound was widened after a run."""
import functools

import numpy as np
import pytest
import torch

import loss_oracle as lo
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = np.float32(np.inf)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _worst(name, err, bound):
    """asserts err <= bound element-wise (err == 0 where the bound is 0) and prints the worst ratio"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    assert np.isfinite(err).all(), name
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print("ratio %-28s %.3f" % (name, ratio))
    assert not err[zero].any(), "%s: a non-zero error where the reference is exactly zero" % name
    assert ratio <= 1.0, "%s: worst err / bound = %.3f" % (name, ratio)
    return ratio


def _same_bits(got_d, got_arg, want_d, want_arg, what):
    got_d, got_arg = host(got_d), host(got_arg)
    assert got_arg.dtype == np.int32 and got_d.dtype == np.float32
    bad = np.argwhere((got_arg != want_arg) | (got_d.view(np.int32) != np.asarray(want_d, np.float32).view(np.int32)))
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got (%r, %d), want (%r, %d)" % (
        what, len(bad), got_arg.size, tuple(bad[0]), got_d[tuple(bad[0])], got_arg[tuple(bad[0])],
        want_d[tuple(bad[0])], want_arg[tuple(bad[0])])


# =============================================================================================== ops.nearest (3-D)
NEAREST_SHAPES = [
    (1, 5, 32769),        # 32 chunks of 1088, the last one EMPTY (it starts at 33728)
    (1, 5, 33729),        # 32 chunks, the last one holds exactly one candidate
    (1, 16, 2047),        # one launch ...
    (1, 16, 2048),        # ... two chunks of 1024
    (64, 256, 4096),      # 1024 groups of 16 queries: one launch
    (63, 256, 4096),      # 1008 groups: two chunks
    (3, 33, 5000),        # Ma % 4 == 1, 4 chunks of 1280
    (2, 1, 1), (1, 3, 63), (1, 17, 65), (2, 4, 257),      # the clamped tail: the last candidate re-read by other lanes
]


@functools.lru_cache(maxsize=None)
def _cloud_case(kind, B, Ma, Nb):
    """(a, b, want_d, want_arg), computed once; the 63-cloud case is the first 63 clouds of the 64-cloud one"""
    if (B, Ma, Nb) == (63, 256, 4096):
        return tuple(x[:63] for x in _cloud_case(kind, 64, Ma, Nb))
    seed = 1000 * B + Ma + Nb
    if kind == "random" and B * Ma * Nb > 1 << 24:
        return lo.cloud_random_rolled(seed, B, Ma, Nb)          # 64 different clouds, torch's answer from 8 of them
    if kind == "random":
        a, b = lo.cloud_random(seed, B, Ma, Nb)
        return (a, b) + lo.nearest_torch(a, b)
    a, b = lo.cloud_lattice(seed, B, Ma, Nb)
    d, arg, tied = lo.nearest_exact_lattice(a, b)
    assert Nb < 2 or tied.mean() >= lo.TIE_SHARE
    return a, b, d, arg


@pytest.mark.parametrize("kind", ["random", "lattice"])
@pytest.mark.parametrize("shape", NEAREST_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_nearest_value_and_first_index_bit_for_bit(shape, kind):
    from usip_amd import ops
    a, b, want_d, want_arg = _cloud_case(kind, *shape)
    d, arg = ops.nearest(dev(a), dev(b))
    _same_bits(d, arg, want_d, want_arg, "%s %s" % (kind, shape))


HAND = (1, 5, 5000)                     # 4 chunks of 1280 (test_loss_oracle_cpu.py::CHUNK_PLANS)


def _far_cloud(seed, B, Ma, Nb):
    """queries within ~0.5 of the origin, candidates on a shell at 3..4: every hand-placed candidate nearer than 2 wins"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, 3, Ma, generator=g) * 0.1
    b = torch.randn(B, 3, Nb, generator=g)
    b = b / b.norm(dim=1, keepdim=True) * (3.0 + torch.rand(B, 1, Nb, generator=g))
    return a, b


def _run_against_torch(a, b, what):
    from usip_amd import ops
    d, arg = ops.nearest(a.to(DEV), b.to(DEV))
    want_d, want_arg = lo.nearest_torch(a, b)
    _same_bits(d, arg, want_d, want_arg, what)
    return host(d), host(arg)


def test_nearest_tie_across_a_chunk_boundary_keeps_the_lower_index():
    """the global minimum duplicated at the last index of one chunk and the first of the next (and further on): the merge
    must keep the lower chunk's; also a duplicate pair whose first member opens a chunk"""
    B, Ma, Nb = HAND
    chunks, chunk = lo.chunk_plan(*HAND)
    assert (chunks, chunk) == (4, 1280)
    a, b = _far_cloud(11, B, Ma, Nb)
    p = torch.tensor([0.5, -0.25, 0.125])
    a[0, :, 0], a[0, :, 1], a[0, :, 4] = torch.eye(3) * 10.0              # three queries far from each other's candidates
    b[0, :, chunk - 1] = b[0, :, chunk] = b[0, :, 3 * chunk + 7] = a[0, :, 0] + p
    b[0, :, 2 * chunk] = b[0, :, 3 * chunk - 1] = b[0, :, 3 * chunk] = a[0, :, 1] - p
    b[0, :, 3 * chunk + 64] = b[0, :, 5] = a[0, :, 4] + 2 * p                 # the LATER chunk is met first in memory order
    d, arg = _run_against_torch(a, b, "chunk-boundary tie")
    assert arg[0, 0] == chunk - 1 and arg[0, 1] == 2 * chunk and arg[0, 4] == 5


@pytest.mark.parametrize("shape", [(1, 3, 63), (2, 4, 257), (1, 17, 65), HAND], ids=lambda s: "%dx%dx%d" % s)
def test_nearest_minimum_only_at_the_last_candidate_and_a_coincident_query(shape):
    """the candidate every clamped lane re-reads is the answer of every query; one query lies ON it: distance exactly 0"""
    B, Ma, Nb = shape
    a, b = _far_cloud(12, B, Ma, Nb)
    b[:, :, Nb - 1] = torch.tensor([0.01, 0.02, 0.03])
    a[0, :, Ma - 1] = b[0, :, Nb - 1]
    d, arg = _run_against_torch(a, b, "last candidate")
    assert (arg == Nb - 1).all() and d[0, Ma - 1] == 0.0 and (d[0, :Ma - 1] > 0).all()


def test_nearest_query_on_a_candidate_gives_exactly_zero():
    B, Ma, Nb = HAND
    a, b = _far_cloud(13, B, Ma, Nb)
    for i, j in enumerate((0, 777, 1280, 2559, 4999)):
        b[0, :, j] = a[0, :, i]
    d, arg = _run_against_torch(a, b, "coincident")
    assert not d.any() and list(arg[0]) == [0, 777, 1280, 2559, 4999]


@pytest.mark.parametrize("order", ["same", "rising", "falling"])
@pytest.mark.parametrize("base", [300, 1280 - 100], ids=["one_chunk", "straddling"])
def test_nearest_ring_inside_the_ambiguity_window(base, order):
    """200 candidates at consecutive indices around query 0 at radii r (1 + k 2^-23), k in 0..3: lanes hold the ring's
    members 64 apart, so most lanes hold two or three candidates whose squares lie within 1 + 2^-20 of the minimum and
    the exact scan decides -- once within chunk 0, once across the boundary of chunks 0 and 1.  k is the same for the
    members of a lane ("same": their squares differ by coordinate rounding only), grows or falls along the lane."""
    B, Ma, Nb = HAND
    a, b = _far_cloud(14, B, Ma, Nb)
    q = torch.tensor([0.3, -0.2, 0.1])
    a[0, :, 0] = q
    i = torch.arange(200)
    k = {"same": i % 4, "rising": i // 64, "falling": 3 - i // 64}[order]
    r = (1.7 * (1.0 + k.double() * 2.0 ** -23))
    th = i.double() * 0.7
    ring = torch.stack((r * torch.cos(th), r * torch.sin(th), torch.zeros(200, dtype=torch.float64))) + q.double()[:, None]
    b[0, :, base:base + 200] = ring.float()
    d, arg = _run_against_torch(a, b, "ring")
    assert base <= arg[0, 0] < base + 200
    s = ((b[0, :, base:base + 200].double() - q.double()[:, None]) ** 2).sum(0)
    inside = (s <= s.min() * (1 + 2.0 ** -20)).view(-1)
    lanes = torch.zeros(64, dtype=torch.int64).index_add_(0, (base + i) % 64, inside.long())
    assert int((lanes >= 2).sum()) >= 16, "the ring no longer puts two candidates of a lane inside the window"


@pytest.mark.parametrize("shape", [(1, 5, 300), HAND], ids=lambda s: "%dx%dx%d" % s)
def test_nearest_overflowing_squares_give_inf_and_index_zero(shape):
    """coordinates of +-1e20: every squared distance is inf, no candidate improves on the start value, and the answer is
    (inf, 0) -- which is what torch.min over torch.norm gives"""
    B, Ma, Nb = shape
    a = torch.full((B, 3, Ma), 1e20)
    b = torch.full((B, 3, Nb), -1e20)
    d, arg = _run_against_torch(a, b, "overflow")
    assert (d == INF).all() and not arg.any()


@pytest.mark.parametrize("shape", [(1, 4, 100), HAND], ids=lambda s: "%dx%dx%d" % s)
def test_nearest_nan_contract(shape):
    """The kernel's OWN contract (csrc/nearest.hip: `sq < best` is false for NaN), not the reference's -- torch.min
    propagates NaN.  A candidate with a NaN coordinate is never selected; a candidate set that is NaN throughout (a whole
    chunk, or everything) and a NaN query give (inf, 0)."""
    from usip_amd import ops
    B, Ma, Nb = shape
    chunks, chunk = lo.chunk_plan(*shape)
    a, b = lo.cloud_random(15, B, Ma, Nb)
    want_d, want_arg = lo.nearest_torch(a, b)
    bad = b.copy()
    dead = np.zeros(Nb, bool)
    dead[want_arg[0]] = True                              # the answers themselves ...
    dead[Nb - 1] = True                                   # ... the candidate the clamped lanes re-read ...
    if chunks > 1:
        dead[chunk:2 * chunk] = True                      # ... and the whole of chunk 1
    bad[0, np.arange(Nb) % 3, np.arange(Nb)] = np.where(dead, np.nan, bad[0, np.arange(Nb) % 3, np.arange(Nb)])
    alive = np.flatnonzero(~dead)
    sub_d, sub_arg = lo.nearest_torch(a, np.ascontiguousarray(bad[:, :, alive]))
    d, arg = ops.nearest(dev(a), dev(bad))
    _same_bits(d, arg, sub_d, alive[sub_arg].astype(np.int32), "NaN candidates")
    qa = a.copy()
    qa[0, 1, 2] = np.nan                                  # one NaN query among sound ones
    d, arg = ops.nearest(dev(qa), dev(b))
    want_d2, want_arg2 = want_d.copy(), want_arg.copy()
    want_d2[0, 2], want_arg2[0, 2] = INF, 0
    _same_bits(d, arg, want_d2, want_arg2, "NaN query")
    d, arg = ops.nearest(dev(a), dev(np.full_like(b, np.nan)))
    _same_bits(d, arg, np.full((B, Ma), INF), np.zeros((B, Ma), np.int32), "all NaN")


# =============================================================================================== ops.nearest_nd
ND_C = (1, 2, 7, 8, 9, 33, 128, 131)
ND_NB = (1, 63, 64, 65, 255, 256, 257, 1023, 1024)
ND_MA = (1, 3, 4, 5, 70)
# every (C, Nb) pair -- so every C meets both templates (Nb <= 256: <4, 8>, else <16, 2>) -- and, Ma walking with both,
# every (C, Ma) and every (Nb, Ma) pair
ND_CASES = [(C, ND_MA[(ci + ni) % 5], Nb) for ci, C in enumerate(ND_C) for ni, Nb in enumerate(ND_NB)]


@pytest.mark.parametrize("C,Ma,Nb", ND_CASES)
def test_nearest_nd_lattice_descriptors_bit_for_bit(C, Ma, Nb):
    from usip_amd import ops
    a, b = lo.desc_lattice(C * 10000 + Ma * 2000 + Nb, 2, C, Ma, Nb)
    want_d, want_arg, tied = lo.nearest_exact_lattice(a, b)
    d, arg = ops.nearest_nd(dev(a), dev(b))
    _same_bits(d, arg, want_d, want_arg, "nd lattice")


@pytest.mark.parametrize("C,Ma,Nb", ND_CASES)
def test_nearest_nd_unit_descriptors_within_the_fma_chain_bounds(C, Ma, Nb):
    """|d - d64| <= (C/2 + 2) 2^-24 d64 and d64[picked] <= min d64 (1 + (C + 4) 2^-24) (loss_oracle.nearest_nd_bounds).
    Measured worst err / bound: value 0.48, index 0.00 (the kernel picked the float64 minimum in every case)."""
    from usip_amd import ops
    a, b = lo.desc_unit(C * 10000 + Ma * 2000 + Nb, 2, C, Ma, Nb)
    d64 = lo.nearest_f64(a, b)
    m64 = d64.min(axis=2)
    d, arg = ops.nearest_nd(dev(a), dev(b))
    d, arg = host(d), host(arg)
    assert arg.dtype == np.int32 and (arg >= 0).all() and (arg < Nb).all()
    val, idx = lo.nearest_nd_bounds(C)
    _worst("nearest_nd value", np.abs(d - m64), val * m64)
    picked = np.take_along_axis(d64, arg[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    _worst("nearest_nd index", picked - m64, idx * m64)


def test_nearest_nd_refuses_more_than_1024_candidates():
    from usip_amd import ops
    a, b = lo.desc_unit(1, 1, 8, 4, 1025)
    with pytest.raises(RuntimeError, match="USIP_EINVAL"):
        ops.nearest_nd(dev(a), dev(b))


# =============================================================================================== ops.nearest_backward
BWD_SHAPES = [
    (2, 3, 40, 47),
    (1, 3, 1300, 70),        # two staging chunks, the second of 276 = a whole number of 16s
    (1, 3, 1029, 64),        # the second chunk holds 5 queries: three of the four quarters are padding
    (2, 5, 100, 130), (1, 6, 17, 3), (1, 7, 2049, 65),        # C % 4 != 0 with a second channel slice
    (2, 128, 256, 256),      # the descriptor loss
    (3, 131, 33, 1),         # one partner takes everything
]


def _forward(ops, a, b):
    return ops.nearest(a, b) if a.shape[1] == 3 else ops.nearest_nd(a, b)


def _bwd_inputs(B, C, Ma, Nb):
    rng = np.random.default_rng(C * 7919 + Ma * 31 + Nb)
    a, b = rng.normal(0, 1, (B, C, Ma)).astype(np.float32), rng.normal(0, 1, (B, C, Nb)).astype(np.float32)
    return a, b, rng.normal(0, 1, (B, Ma)).astype(np.float32)


def _distance_to(a, b, arg):
    """float32 of the float64 distance to a GIVEN partner: what the forward would have saved, to one rounding"""
    sel = np.take_along_axis(b.astype(np.float64), np.broadcast_to(arg[:, None, :].astype(np.int64), a.shape), axis=2)
    return np.sqrt(((a.astype(np.float64) - sel) ** 2).sum(axis=1)).astype(np.float32)


@pytest.mark.parametrize("variant", ["own", "all_to_last", "lower_half"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_nearest_backward_matches_float64_at_equal_decisions(shape, variant):
    """own: the forward's (d, arg); all_to_last: every query sent to partner Nb - 1 (a sum of Ma terms, every staging chunk
    and quarter contributing); lower_half: the upper half of the partners is nobody's -- their gb is exactly zero, not
    merely small.  Bounds: loss_oracle.nearest_backward_f64.  Measured worst err / bound: ga 0.36, gb 0.18."""
    from usip_amd import ops
    B, C, Ma, Nb = shape
    a, b, gd = _bwd_inputs(*shape)
    if variant == "own":
        d, arg = _forward(ops, dev(a), dev(b))
    else:
        rng = np.random.default_rng(Ma)
        half = (Nb + 1) // 2
        arg_h = np.full((B, Ma), Nb - 1) if variant == "all_to_last" else rng.integers(0, half, (B, Ma))
        arg_h = arg_h.astype(np.int32)
        d, arg = dev(_distance_to(a, b, arg_h)), dev(arg_h)
    ga, gb = ops.nearest_backward(dev(a), dev(b), d, arg, dev(gd), True)
    ga, gb = host(ga), host(gb)
    rga, rgb, n, S = lo.nearest_backward_f64(a, b, host(arg), gd)
    bga, bgb = lo.nearest_backward_bounds(C, gd, n, S)
    _worst("nearest_bwd ga", np.abs(ga - rga), bga)
    _worst("nearest_bwd gb", np.abs(gb - rgb), bgb)
    assert not gb[np.broadcast_to((n == 0)[:, None, :], gb.shape)].any()         # nobody's partner: 0.0 (either sign of zero)
    if variant == "lower_half" and Nb > 1:
        assert (n[:, (Nb + 1) // 2:] == 0).all() and not gb[:, :, (Nb + 1) // 2:].any()
    if variant == "all_to_last":
        assert (n[:, Nb - 1] == Ma).all()


def test_nearest_backward_zero_distance_no_gb_and_determinism():
    """a query ON its partner: its ga row is exactly zero (the sub-gradient of torch.norm at zero); need_gb=False returns
    None and the same ga; a second launch gives the same bits of ga and gb"""
    from usip_amd import ops
    for shape in ((2, 3, 1300, 70), (2, 7, 100, 130)):
        a, b, gd = _bwd_inputs(*shape)
        a[1, :, 9] = b[1, :, 5]
        A, Bt, G = dev(a), dev(b), dev(gd)
        d, arg = _forward(ops, A, Bt)
        assert float(d[1, 9]) == 0.0 and int(arg[1, 9]) == 5
        ga, gb = ops.nearest_backward(A, Bt, d, arg, G, True)
        assert not host(ga)[1, :, 9].any() and host(ga)[1, :, 8].all()
        ga2, none = ops.nearest_backward(A, Bt, d, arg, G, False)
        assert none is None and torch.equal(ga2, ga)
        ga3, gb3 = ops.nearest_backward(A, Bt, d, arg, G, True)
        assert torch.equal(ga3, ga) and torch.equal(gb3, gb)


# =============================================================================================== ops.chamfer_prob
CHAMFER_SHAPES = [
    (1, 1, 1), (2, 64, 64), (1, 63, 65), (4, 1023, 1),
    (4, 1024, 1024),         # 4 * 1024 values: the unrolled loop runs zero times, the tail takes everything
    (4, 1025, 1024),         # the first thread runs the unrolled loop once
    (3, 1024, 1025), (5, 1023, 2049),
    (16, 512, 512),          # the training step's own
]
GLOSS = (0.7, -2.0, 0.0)


@pytest.mark.parametrize("pattern", lo.CHAMFER_PATTERNS)
@pytest.mark.parametrize("shape", CHAMFER_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_chamfer_prob_forward_and_backward_match_float64(shape, pattern):
    """Both sigma regimes (uniform in [0.05, 1.5]; all at 1e-3 with distances up to 100) and the three upstream gradients
    against loss_oracle.chamfer_f64 at its bounds: loss 8 U of the summed magnitudes, pure and weighted 8 U relative,
    da / dc 4 U per element, dss / dsd (n_t + 8) U of the summed magnitudes H_t; gloss = 0 gives zeros.
    Measured worst err / bound: loss 0.17, pure 0.25, weighted 0.16, da 0.71, dc 0.80, dss 0.46, dsd 0.45."""
    from usip_amd import ops
    B, M, N = shape
    for tiny in (False, True):
        a, J, c, I, ss, sd = lo.chamfer_inputs(B * 100000 + M * 10 + N, B, M, N, pattern, tiny)
        if pattern == "all_to_one":
            assert not J.any() and (I == M - 1).all()
        t = [dev(x) for x in (a, J, c, I, ss, sd)]
        out = host(ops.chamfer_prob(*t))
        for g in GLOSS:
            g32 = np.float32(g)
            r = lo.chamfer_f64(a, J, c, I, ss, sd, float(g32))
            if g == GLOSS[0]:
                tag = "tiny" if tiny else "unit"
                _worst("chamfer loss %s" % tag, abs(out[0] - r["loss"]), 8 * lo.U * r["loss_mag"])
                _worst("chamfer pure %s" % tag, abs(out[1] - r["pure"]), 8 * lo.U * abs(r["pure"]))
                _worst("chamfer weighted %s" % tag, abs(out[2] - r["weighted"]), 8 * lo.U * abs(r["weighted"]))
            da, dc, dss, dsd = (host(x) for x in ops.chamfer_prob_backward(torch.tensor(g32, device=DEV), *t))
            _worst("chamfer da", np.abs(da - r["da"]), 4 * lo.U * np.abs(r["da"]))
            _worst("chamfer dc", np.abs(dc - r["dc"]), 4 * lo.U * np.abs(r["dc"]))
            _worst("chamfer dss", np.abs(dss - r["dss"]), (r["n_ss"] + 8) * lo.U * r["H_ss"])
            _worst("chamfer dsd", np.abs(dsd - r["dsd"]), (r["n_sd"] + 8) * lo.U * r["H_sd"])
            if g == 0.0:
                assert not (da.any() or dc.any() or dss.any() or dsd.any())


def test_chamfer_prob_backward_is_deterministic_and_refuses_65536_pairs():
    from usip_amd import ops
    t = [dev(x) for x in lo.chamfer_inputs(5, 5, 1023, 2049, "first40")]
    gl = torch.tensor(0.7, device=DEV)
    first = ops.chamfer_prob_backward(gl, *t)
    for x, y in zip(first, ops.chamfer_prob_backward(gl, *t)):
        assert torch.equal(x, y)
    big = [dev(x) for x in lo.chamfer_inputs(6, 65536, 1, 1, "identity")]
    out = host(ops.chamfer_prob(*big))                                  # the forward has no such limit
    r = lo.chamfer_f64(*lo.chamfer_inputs(6, 65536, 1, 1, "identity"), 1.0)
    _worst("chamfer loss 65536", abs(out[0] - r["loss"]), 8 * lo.U * r["loss_mag"])
    with pytest.raises(RuntimeError, match="USIP_EINVAL"):
        ops.chamfer_prob_backward(gl, *big)


# =============================================================================================== through the modules
MODULE_SHAPES = [(1, 1, 1), (2, 1, 700), (2, 513, 40), (1, 16, 2048)]


class _DropGrad(torch.autograd.Function):
    """passes its input on and returns NO gradient for it: the producer's backward then runs with gd = None"""

    @staticmethod
    def forward(ctx, x, keep):
        return x.view_as(x), keep.view_as(keep)

    @staticmethod
    def backward(ctx, gx, gkeep):
        return None, gkeep


@pytest.mark.parametrize("shape", MODULE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_chamfer_loss_module_matches_float64_at_equal_arg_minima(shape):
    """losses.ChamferLoss_Brute through autograd against the float64 restatement of models/losses.py:59-99 at the module's
    own arg-minima (which are the oracle's, bit for bit): the suite's bar, 1e-5 of each tensor's scale"""
    from usip_amd import losses
    from usip_amd.networks import DetectorOptions
    B, M, N = shape
    src, dst = lo.cloud_random(B + M + N, B, M, N)
    rng = np.random.default_rng(M)
    ss, sd = rng.uniform(0.05, 1.5, (B, M)).astype(np.float32), rng.uniform(0.05, 1.5, (B, N)).astype(np.float32)
    t = [dev(x).requires_grad_(True) for x in (src, dst, ss, sd)]
    crit = losses.ChamferLoss_Brute(DetectorOptions())
    loss, pure, weighted = crit(*t)
    assert not pure.requires_grad and not weighted.requires_grad
    loss.backward()
    J, I = (host(x) for x in crit.last_indices)
    assert np.array_equal(J, lo.nearest_torch(src, dst)[1]) and np.array_equal(I, lo.nearest_torch(dst, src)[1])
    r = lo.chamfer_module_f64(src, dst, ss, sd, J, I)
    for got, key in ((loss, "loss"), (pure, "pure"), (weighted, "weighted")):
        assert_close(host(got), np.float64(r[key]), name=key)
    for got, key in zip(t, ("gsrc", "gdst", "gss", "gsd")):
        assert_close(host(got.grad), r[key], name=key)


@pytest.mark.parametrize("shape", MODULE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_keypoint_on_pc_module_gradient_wiring(shape, monkeypatch):
    """losses.KeypointOnPCLoss (point to point) through autograd: the cloud carries no gradient (no gb is formed), only the
    cloud carries one (ga is dropped), and a distance nobody differentiates (gd is None) yields no gradient at all"""
    from usip_amd import functional as Fh
    from usip_amd import losses
    from usip_amd.networks import DetectorOptions
    B, M, N = shape
    kp, pc = lo.cloud_random(7 * (B + M + N), B, M, N)
    gd = np.random.default_rng(N).normal(0, 1, (B, M)).astype(np.float32)
    crit = losses.KeypointOnPCLoss(DetectorOptions())
    want_d, want_arg = lo.nearest_torch(kp, pc)
    rd, rga = lo.single_side_f64(kp, pc, want_arg, gd)
    _, rgb, _, _ = lo.nearest_backward_f64(kp, pc, want_arg, gd)
    K, P = dev(kp).requires_grad_(True), dev(pc)
    d = crit(K, P, None)
    assert np.array_equal(host(d), want_d)
    d.backward(dev(gd))
    assert P.grad is None
    assert_close(host(K.grad), rga, name="d/dkp")
    K, P = dev(kp), dev(pc).requires_grad_(True)                       # needs_input_grad = (False, True)
    crit(K, P, None).backward(dev(gd))
    assert K.grad is None
    assert_close(host(P.grad), rgb, name="d/dpc")
    K, P = dev(kp).requires_grad_(True), dev(pc).requires_grad_(True)   # both, and an output without a gradient
    from usip_amd import ops
    launches, real = [], ops.nearest_backward
    monkeypatch.setattr(ops, "nearest_backward", lambda *args: launches.append(1) or real(*args))
    d, arg = Fh.nearest_distance_i32(K, P)
    assert np.array_equal(host(arg), want_arg) and not arg.requires_grad
    other = (K * 2.0).sum(dim=1)
    dropped, kept = _DropGrad.apply(d, other)
    (dropped.sum() + kept.sum()).backward()
    assert not launches and P.grad is None and torch.equal(K.grad, torch.full_like(K, 2.0))
