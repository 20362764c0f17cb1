"""The CGF triplet loss's host twin (csrc/cgf_loss_cpu.cpp over csrc/cgf_math.h; include/usip_hip.h f-22) against the
reference's own DescCGFLoss (tests/golden/cgf_loss_cases.npz, written by tests/golden/make_cgf_golden.py), against the
independent oracle (tests/cgf_oracle.py), and a stand-alone sanitizer build.  The device is held to this twin bit for bit in
tests/test_cgf_loss_gpu.py, which borrows the inputs.

  1 fixture     the twin on the recorded draws: the reference's indices EQUAL; loss, active and the descriptor gradients of
                loss.mean() at the project's 1e-5 (conftest.assert_close).
  2 oracle      the oracle adds in the contract's orders with IEEE float64 operations, so it is held to EQUALITY, on the
                fixture's inputs and on exact-operand cases: a point ON the radius (difference (3, 4, 0), radius 5: positive,
                never "outside"); an anchor descriptor equal to its positive (zero distance, zero unit vector, nothing
                non-finite); every sigma at or above sigma_max (a zero row: the stated deviation from the reference's NaN);
                all M anchors sharing one j_neg (the longest ordered sum of d_pos).
  3 refusals    every limit one step inside and one step outside; NULL pointers; some but not all of the draws.
  4 Philox      the counter layout against a Philox written on python integers; a selection depends on (seed, step, global
                element) only, whatever B, elem_base and num_threads; a chosen positive is inside the radius, a chosen j_out
                outside whenever an outside point exists, j_far the brute-force float32 arg-min; and a derived uniformity
                bound: an anchor with exactly two positives takes the first 2048 +- 192 times in 4096 steps (six standard
                deviations of Binomial(4096, 1/2), sigma = 32).
  5 module      losses.DescCGFLoss on host tensors: the fixture again through autograd, the step counter, last_indices.
  6 sanitizers  tests/cgf_sanitize_main.cpp."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cgf_oracle as co
from conftest import ROOT, assert_close, load_golden
from usip_amd import ops

CASES = ("batch3", "single", "surface", "wide")
INPUTS = ("anc_kp", "pos_kp", "anc_desc", "pos_desc", "anc_sigma")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# a host compiler: g++ or clang++ where there is one, otherwise the clang++ beside hipcc, which every build here needs anyway
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")
F = np.float32


@functools.lru_cache(maxsize=None)
def fixture(name):
    """one case of the reference fixture without its prefix; nobody writes into it"""
    g = load_golden("cgf_loss_cases.npz")
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_")}


def tens(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def draws_of(c):
    return None if c.get("u1") is None else {k: tens(c[k]) for k in ("u1", "u2", "u3")}


def run_twin(c, num_threads=3, grad=None, seed=0, step=0, elem_base=0):
    """the twin on a case dict (numpy) -> dict of numpy arrays: sel, has, take_far, loss, active, dist, coef, d_anc, d_pos"""
    t = {k: tens(c[k]) for k in INPUTS}
    sel, has, take_far = ops.cgf_select_cpu(t["anc_kp"], t["pos_kp"], float(c["radius"]), draws_of(c), seed, step, elem_base,
                                            num_threads)
    loss, active, dist, coef = ops.cgf_loss_cpu(t["anc_desc"], t["pos_desc"], t["anc_sigma"], sel, has, take_far,
                                                float(c["gamma"]), float(c["sigma_max"]), num_threads)
    g = tens(grad_of(c) if grad is None else grad)
    d_anc, d_pos = ops.cgf_loss_backward_cpu(t["anc_desc"], t["pos_desc"], sel, take_far, dist, coef, g, num_threads)
    return {k: v.numpy() for k, v in dict(sel=sel, has=has, take_far=take_far, loss=loss, active=active, dist=dist, coef=coef,
                                          d_anc=d_anc, d_pos=d_pos).items()}


def grad_of(c):
    """the gradient loss.mean() sends back: 1 / (B M) everywhere"""
    B, _, M = c["anc_kp"].shape
    return np.full((B, M), 1.0 / (B * M), F)


def run_oracle(c, grad=None):
    sel, has, take_far = co.select(c["anc_kp"], c["pos_kp"], float(c["radius"]), c["u1"], c["u2"], c["u3"])
    out = co.loss(c["anc_desc"], c["pos_desc"], c["anc_sigma"], sel, has, take_far, float(c["gamma"]), float(c["sigma_max"]))
    d_anc, d_pos = co.backward(c["anc_desc"], c["pos_desc"], sel, take_far, out["dist"], out["coef"],
                               grad_of(c) if grad is None else grad)
    return dict(out, sel=sel, has=has, take_far=take_far, d_anc=d_anc, d_pos=d_pos)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_same_bits(got, want, names=None, tag=""):
    for k in names or sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s %s: %d of %d differ" % (
            tag, k, int((bits(got[k]) != bits(want[k])).sum()), got[k].size)


OUTPUTS = ("sel", "has", "take_far", "loss", "active", "dist", "coef", "d_anc", "d_pos")


# ---------------------------------------------------------------------------------------------------- exact-operand cases
def _case(anc_kp, pos_kp, anc_desc, pos_desc, anc_sigma, radius, gamma, sigma_max, seed):
    B, _, M = anc_kp.shape
    g = np.random.default_rng(seed)
    u = lambda *s: ((g.integers(1, 1 << 24, s)).astype(F) * F(2.0 ** -24))      # noqa: E731   24-bit uniforms, never 0
    return dict(anc_kp=anc_kp.astype(F), pos_kp=pos_kp.astype(F), anc_desc=anc_desc.astype(F), pos_desc=pos_desc.astype(F),
                anc_sigma=anc_sigma.astype(F), radius=radius, gamma=gamma, sigma_max=sigma_max, u1=u(B, M, M), u2=u(B, M, M),
                u3=u(B, M))


def _lattice(B, M):
    """anchors 10 apart along x, positive i at its anchor + (3, 4, 0): d_ii = 5 exactly, every other d_ij is not 5"""
    anc = np.zeros((B, 3, M))
    anc[:, 0, :] = 10.0 * np.arange(M)
    anc[:, 1, :] = np.arange(B)[:, None]
    pos = anc + np.array([3.0, 4.0, 0.0])[None, :, None]
    return anc, pos


@functools.lru_cache(maxsize=None)
def exact_case(name, M=5, C=3, B=2):
    g = np.random.default_rng(5)
    ints = lambda *s: g.integers(-4, 5, s).astype(np.float64)                    # noqa: E731
    sig = g.integers(0, 6, (B, M)) * 0.25                                       # quarters: exact; some at or above sigma_max 1
    if name == "on_radius":
        anc, pos = _lattice(B, M)
        return _case(anc, pos, ints(B, C, M), ints(B, C, M), sig, 5.0, 0.5, 1.0, 1)
    if name == "equal_desc":            # the positive's descriptor IS the anchor's; gamma keeps the triplet active all the same
        anc, pos = _lattice(B, M)
        d = ints(B, C, M)
        return _case(anc, pos, d, d.copy(), sig, 5.0, 64.0, 1.0, 2)
    if name == "dead_sigma":            # element 0: every sigma at or above sigma_max
        anc, pos = _lattice(B, M)
        sig = sig.copy()
        sig[0] = 1.0 + 0.25 * (np.arange(M) % 3)
        sig[1:, 0] = 0.25
        return _case(anc, pos, ints(B, C, M), ints(B, C, M), sig, 5.0, 64.0, 1.0, 3)
    if name == "shared_neg":            # one point outside the radius: every anchor's j_far and j_out
        anc = np.zeros((B, 3, M))
        anc[:, 0, :] = np.arange(M) % 4
        pos = anc.copy()
        pos[:, :, M // 2] = 100.0
        return _case(anc, pos, ints(B, C, M), ints(B, C, M), np.full((B, M), 0.25), 5.0, 64.0, 1.0, 4)
    raise KeyError(name)


EXACT = ("on_radius", "equal_desc", "dead_sigma", "shared_neg")


# ---------------------------------------------------------------------------------------------------- 1: the reference fixture
@pytest.mark.parametrize("name", CASES)
def test_twin_matches_the_reference_fixture(name):
    c = fixture(name)
    got = run_twin(c)
    assert np.array_equal(got["sel"], c["sel"])                         # the reference's own three indices
    assert np.array_equal(got["has"], c["has"]) and np.array_equal(got["take_far"], c["take_far"])
    assert_close(got["loss"], c["loss"], name=name + " loss")
    assert_close(got["active"], c["active"], name=name + " active")
    assert_close(got["d_anc"], c["d_anc"], name=name + " d_anc")
    assert_close(got["d_pos"], c["d_pos"], name=name + " d_pos")


def test_fixture_holds_the_elements_it_names():
    c = fixture("batch3")
    n = c["has"].sum(1)
    assert 0 < n[0] < 48 and n[1] == 0 and n[2] == 48
    assert (c["loss"][1] == 0).all() and c["active"][1] == 0            # nothing matched: an empty row
    assert (c["sel"][1, :, 0] == 0).all() and (c["sel"][2, :, 2] == 0).all()      # all-zero rows give index 0
    assert fixture("single")["anc_kp"].shape == (2, 3, 1)
    assert float(fixture("surface")["radius"]) == 0.075 and float(fixture("wide")["radius"]) == 5.0
    for name in CASES:
        assert float(fixture(name)["margin"]) >= 1e-3 and min(float(fixture(name)[k].min()) for k in ("u1", "u2", "u3")) > 0


# ---------------------------------------------------------------------------------------------------- 2: the oracle
@pytest.mark.parametrize("name", CASES + EXACT)
def test_twin_equals_the_oracle(name):
    c = fixture(name) if name in CASES else exact_case(name)
    assert_same_bits(run_twin(c), run_oracle(c), OUTPUTS, name)


def test_thread_counts_agree():
    c = fixture("batch3")
    one = run_twin(c, 1)
    for nt in (2, 7, 64):
        assert_same_bits(run_twin(c, nt), one, OUTPUTS, "threads %d" % nt)


def test_a_point_on_the_radius_is_positive_and_never_outside():
    c = exact_case("on_radius")
    got = run_twin(c)
    M = c["anc_kp"].shape[2]
    assert (got["has"] == 1).all()
    assert (got["sel"][:, :, 0] == np.arange(M)).all()                  # the one positive of anchor i is point i, at d == 5
    assert (got["sel"][:, :, 1] != np.arange(M)).all() and (got["sel"][:, :, 2] != np.arange(M)).all()


def test_zero_distance_gives_a_zero_unit_vector_and_nothing_non_finite():
    c = exact_case("equal_desc")
    got = run_twin(c)
    assert (got["dist"][:, :, 0] == 0).all() and (got["coef"] > 0).any()
    for k in ("loss", "active", "dist", "coef", "d_anc", "d_pos"):
        assert np.isfinite(got[k]).all(), k
    # only the negative's unit vector is left in d_anc
    jn = co.negatives(got["sel"], got["take_far"])
    g = grad_of(c).astype(np.float64) * got["coef"]
    for b in range(c["anc_kp"].shape[0]):
        for i in range(c["anc_kp"].shape[2]):
            v = c["anc_desc"][b, :, i].astype(np.float64) - c["pos_desc"][b, :, jn[b, i]].astype(np.float64)
            dn = got["dist"][b, i, 1]
            want = g[b, i] * (0.0 - v / dn) if dn > 0 else np.zeros_like(v)
            assert np.array_equal(got["d_anc"][b, :, i], want.astype(F))


def test_every_sigma_at_or_above_sigma_max_gives_a_zero_row():
    c = exact_case("dead_sigma")
    got = run_twin(c)
    assert (got["loss"][0] == 0).all() and (got["coef"][0] == 0).all() and (got["d_anc"][0] == 0).all()
    assert (got["loss"][1] > 0).any() and np.isfinite(got["loss"]).all() and np.isfinite(got["active"]).all()
    assert got["active"][0] > 0                                         # the triplets are active; only their weight is 0


@pytest.mark.parametrize("M,C", [(130, 3), (7, 130)])
def test_all_anchors_sharing_one_negative(M, C):
    c = exact_case("shared_neg", M, C)
    got = run_twin(c, 4)
    k = M // 2
    assert (co.negatives(got["sel"], got["take_far"]) == k).all()       # the longest ordered sum: M terms in one column
    assert_same_bits(got, run_oracle(c), OUTPUTS, "shared_neg")
    assert (got["d_pos"][:, :, k] != 0).any()


def test_indices_read_from_memory_are_clamped():
    c = fixture("single")
    t = {k: tens(c[k]) for k in INPUTS}
    sel = torch.tensor([[[7, -3, 99]], [[-1, 1 << 30, 5]]], dtype=torch.int32)
    has, tf = torch.ones((2, 1), dtype=torch.uint8), torch.tensor([[1], [0]], dtype=torch.uint8)
    zero = torch.zeros((2, 1, 3), dtype=torch.int32)
    a = ops.cgf_loss_cpu(t["anc_desc"], t["pos_desc"], t["anc_sigma"], sel, has, tf, 0.5, 1.0)
    b = ops.cgf_loss_cpu(t["anc_desc"], t["pos_desc"], t["anc_sigma"], zero, has, tf, 0.5, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 3: refusals
def test_the_library_refuses_null_pointers_and_limits():
    from usip_amd import _lib
    L = _lib.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                        # noqa: E731
    kp, u2d, u1d = np.zeros((1, 3, 2), F), np.full((1, 2, 2), 0.5, F), np.full((1, 2), 0.5, F)
    sel, has, tf = np.zeros((1, 2, 3), np.int32), np.zeros((1, 2), np.uint8), np.zeros((1, 2), np.uint8)
    ok = [p(kp), p(kp), 1, 2, 1.0, None, None, None, 0, 0, 0, p(sel), p(has), p(tf), 1]
    assert L.usip_cgf_select_f32_cpu(*ok) == 0
    for i, bad in ((0, None), (1, None), (11, None), (12, None), (13, None), (2, 0), (2, -1), (3, 0), (3, 65536), (4, 0.0),
                   (4, -1.0), (4, float("nan")), (4, 1e-60), (5, p(u2d)), (6, p(u2d)), (7, p(u1d))):
        args = list(ok)
        args[i] = bad
        assert L.usip_cgf_select_f32_cpu(*args) < 0, i
    args = list(ok)
    args[4], args[5], args[6], args[7] = 1e-30, p(u2d), p(u2d), p(u1d)  # inside: a tiny radius, all three draws
    assert L.usip_cgf_select_f32_cpu(*args) == 0

    def loss_args(M, C):
        d, s = np.zeros((1, C, M), F), np.zeros((1, M), F)
        keep = [d, s, np.zeros((1, M, 3), np.int32), np.zeros((1, M), np.uint8), np.zeros((1, M), F), np.zeros((1,), F),
                np.zeros((1, M, 2)), np.zeros((1, M))]
        return keep, [p(d), p(d), p(s), p(keep[2]), p(keep[3]), p(keep[3]), 1, M, C, 0.5, 1.0, p(keep[4]), p(keep[5]),
                      p(keep[6]), p(keep[7]), 2]

    # the limits themselves are inside (M = 65535 on the loss entry: the shape test is one function, csrc/cgf_math.h's bad_shape,
    # and an all-pairs selection of 65535 anchors on the host would take minutes)
    for M, C in ((1, 1), (65535, 1), (1, 4096)):
        keep, args = loss_args(M, C)
        assert L.usip_cgf_loss_f32_cpu(*args) == 0, (M, C)
    keep, ok = loss_args(2, 2)
    for i, bad in [(i, None) for i in (0, 1, 2, 3, 4, 5, 11, 12, 13, 14)] + [(6, 0), (7, 0), (7, 65536), (8, 0), (8, 4097)]:
        args = list(ok)
        args[i] = bad
        assert L.usip_cgf_loss_f32_cpu(*args) < 0, i
    d, g = np.zeros((1, 2, 2), F), np.zeros((1, 2), F)
    ok = [p(d), p(d), p(keep[2]), p(keep[3]), p(keep[6]), p(keep[7]), p(g), 1, 2, 2, p(d.copy()), p(d.copy()), 1]
    outs = [np.zeros((1, 2, 2), F), np.zeros((1, 2, 2), F)]
    ok[10], ok[11] = p(outs[0]), p(outs[1])
    assert L.usip_cgf_loss_backward_f32_cpu(*ok) == 0
    for i, bad in [(i, None) for i in (0, 1, 2, 3, 4, 5, 6, 10, 11)] + [(7, 0), (8, 0), (8, 65536), (9, 0), (9, 4097)]:
        args = list(ok)
        args[i] = bad
        assert L.usip_cgf_loss_backward_f32_cpu(*args) < 0, i
    # the device entry points refuse the same things before they launch anything
    assert L.usip_cgf_select_f32(None, None, 1, 2, 1.0, None, None, None, 0, 0, None, 0, None, None, None, None) < 0
    assert L.usip_cgf_select_f32(p(kp), p(kp), 1, 65536, 1.0, None, None, None, 0, 0, None, 0, p(sel), p(has), p(tf), None) < 0
    assert L.usip_cgf_loss_f32(*loss_args(2, 4097)[1][:15], None) < 0
    assert L.usip_cgf_loss_backward_f32(*ok[:9], 4097, ok[10], ok[11], None) < 0


def test_wrappers_refuse_wrong_tensors():
    c = fixture("single")
    t = {k: tens(c[k]) for k in INPUTS}
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.cgf_select(t["anc_kp"], t["pos_kp"], 1.0)                   # the device wrapper takes no host tensor
    with pytest.raises(RuntimeError):
        ops.cgf_select_cpu(t["anc_kp"].double(), t["pos_kp"], 1.0)
    with pytest.raises(RuntimeError):
        ops.cgf_select_cpu(t["anc_kp"], t["pos_kp"], 0.0)
    with pytest.raises(RuntimeError):
        ops.cgf_select_cpu(t["anc_kp"], t["pos_kp"], 1.0, dict(u1=tens(c["u1"]), u2=tens(c["u2"]), u3=tens(c["u1"])))


# ---------------------------------------------------------------------------------------------------- 4: Philox
def _cloud(seed, B, M, radius=1.0):
    g = np.random.default_rng(seed)
    anc = g.uniform(-2, 2, (B, 3, M)).astype(F)
    pos = (anc + g.uniform(-1, 1, (B, 3, M)) * np.where(np.arange(M) % 2 == 0, 0.4, 3.0) * radius).astype(F)
    return anc, pos


def test_counter_layout_against_an_independent_philox():
    B, M, seed, step, base = 2, 9, 11, 3, 4
    anc, pos = _cloud(1, B, M)
    got = ops.cgf_select_cpu(tens(anc), tens(pos), 1.0, None, seed, step, base, 2)
    u = [co.philox_draws(seed, step, base + b, M) for b in range(B)]
    draws = {k: tens(np.stack([x[n] for x in u])) for n, k in enumerate(("u1", "u2", "u3"))}
    assert 0.0 <= float(draws["u1"].min()) and float(draws["u1"].max()) < 1.0
    want = ops.cgf_select_cpu(tens(anc), tens(pos), 1.0, draws)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(got, co.select(anc, pos, 1.0, *[d.numpy() for d in draws.values()])))


def test_a_draw_depends_on_seed_step_and_global_element_only():
    B, M = 4, 33
    anc, pos = _cloud(2, B, M)
    whole = ops.cgf_select_cpu(tens(anc), tens(pos), 1.0, None, 7, 5, 10, 1)
    for b in range(B):                                                  # one element at a time, any thread count
        part = ops.cgf_select_cpu(tens(anc[b:b + 1]), tens(pos[b:b + 1]), 1.0, None, 7, 5, 10 + b, 1 + 2 * b)
        assert all(torch.equal(x[b:b + 1], y) for x, y in zip(whole, part))
    halves = ops.cgf_select_cpu(tens(anc[2:]), tens(pos[2:]), 1.0, None, 7, 5, 12, 5)       # a rank's share
    assert all(torch.equal(x[2:], y) for x, y in zip(whole, halves))
    for other in (dict(seed=8, step=5), dict(seed=7, step=6)):          # and on each of them
        o = ops.cgf_select_cpu(tens(anc), tens(pos), 1.0, None, other["seed"], other["step"], 10, 1)
        assert not torch.equal(o[0], whole[0])
    moved = ops.cgf_select_cpu(tens(anc), tens(pos), 1.0, None, 7, 5, 11, 1)
    assert not torch.equal(moved[0], whole[0])


def test_philox_selections_hold_the_contracts_properties():
    B, M, r = 3, 64, 1.0
    anc, pos = _cloud(3, B, M)
    d = co.distances(anc, pos)
    inside, outside = d <= F(r), d > F(r)
    far = np.argmin(d + np.where(inside, F(1000), F(0)), axis=2)
    seen = set()
    for step in range(8):
        sel, has, tf = [x.numpy() for x in ops.cgf_select_cpu(tens(anc), tens(pos), r, None, 1, step, 0, 2)]
        bi, ii = np.nonzero(has)
        assert np.array_equal(has != 0, inside.any(2))
        assert inside[bi, ii, sel[bi, ii, 0]].all()                     # a chosen positive is inside the radius
        bo, io = np.nonzero(outside.any(2))
        assert outside[bo, io, sel[bo, io, 2]].all()                    # a chosen j_out is outside whenever one exists
        assert np.array_equal(sel[:, :, 1], far)                        # j_far is the brute-force float32 arg-min
        seen.add(sel[:, :, 0].tobytes())
    assert len(seen) == 8                                               # every step draws anew


def test_two_positives_are_taken_evenly():
    """Binomial(4096, 1/2): mean 2048, sigma 32; the bar is six sigma.  Nothing here is fitted to the generator."""
    anc = np.zeros((1, 3, 3), F)
    anc[0, 0] = [0, 50, 100]
    pos = anc.copy()
    pos[0, :, 0], pos[0, :, 1] = [0.1, 0, 0], [0, 0.1, 0]               # anchor 0: points 0 and 1 inside, point 2 far away
    a, p = tens(anc), tens(pos)
    first = far = 0
    for step in range(4096):
        sel, has, tf = ops.cgf_select_cpu(a, p, 1.0, None, 2024, step)
        assert has[0, 0] == 1 and int(sel[0, 0, 0]) in (0, 1)
        first += int(sel[0, 0, 0]) == 0
        far += int(tf[0, 0])
    assert abs(first - 2048) <= 192, first
    assert abs(far - 2048) <= 192, far                                  # the coin between j_far and j_out, by the same bound


# ---------------------------------------------------------------------------------------------------- 5: the module
class Opt:
    def __init__(self, c):
        self.CGF_radius, self.triple_loss_gamma, self.sigma_max = float(c["radius"]), float(c["gamma"]), float(c["sigma_max"])


@pytest.mark.parametrize("name", CASES)
def test_module_on_host_tensors_matches_the_fixture(name):
    from usip_amd.losses import DescCGFLoss
    c = fixture(name)
    t = {k: tens(c[k]) for k in INPUTS}
    t["anc_desc"].requires_grad_(True)
    t["pos_desc"].requires_grad_(True)
    mod = DescCGFLoss(Opt(c))
    loss, active = mod(t["anc_kp"], t["anc_desc"], t["pos_kp"], t["pos_desc"], t["anc_sigma"], None, None, draws=draws_of(c))
    loss.mean().backward()
    assert loss.shape == c["loss"].shape and active.shape == c["active"].shape
    assert np.array_equal(mod.last_indices[0].numpy(), c["sel"])
    assert_close(loss.detach().numpy(), c["loss"], name="loss")
    assert_close(active.numpy(), c["active"], name="active")
    assert_close(t["anc_desc"].grad.numpy(), c["d_anc"], name="d_anc")
    assert_close(t["pos_desc"].grad.numpy(), c["d_pos"], name="d_pos")
    assert t["anc_kp"].grad is None and t["anc_sigma"].grad is None


def test_module_steps_its_counter_in_training_only():
    from usip_amd.losses import DescCGFLoss
    c = fixture("batch3")
    t = [tens(c[k]) for k in ("anc_kp", "anc_desc", "pos_kp", "pos_desc", "anc_sigma")]
    mod = DescCGFLoss(Opt(c), seed=3)
    mod(*t)
    a = mod.last_indices
    mod(*t)
    b = mod.last_indices
    assert not torch.equal(a[0], b[0])                                  # training: the next step's draws
    mod.eval()
    mod(*t)
    e1 = mod.last_indices
    mod(*t)
    assert torch.equal(e1[0], mod.last_indices[0])                      # evaluation: the counter stands
    mod(*t, step=0)
    assert torch.equal(a[0], mod.last_indices[0])                       # an explicit step reproduces a call
    want = ops.cgf_select_cpu(t[0], t[2], float(c["radius"]), None, 3, 1)
    assert torch.equal(b[0], want[0]) and torch.equal(b[2], want[2])


# ---------------------------------------------------------------------------------------------------- 6: the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "cgf_sanitize_main.cpp")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/cgf_loss_cpu.cpp: random elements, M and C at and around the lane and
    workgroup widths, explicit and Philox draws, indices out of range, non-finite coordinates and descriptors.  It links
    nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "cgf_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "cgf_loss_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
