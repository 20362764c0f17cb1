"""The CGF triplet loss on the device (csrc/cgf_loss.hip; include/usip_hip.h f-22) against its host twin, bit for bit, against
the reference's own DescCGFLoss (tests/golden/cgf_loss_cases.npz) and, through the module, against a dense torch-double
restatement of the reference's formulation.  Inputs and helpers are tests/test_cgf_loss_cpu.py's.

  1 twin       sel, has, take_far, loss, active, dist, coef, d_anc and d_pos EQUAL the twin's as bit patterns, on explicit
               draws and on Philox, over M in {1, 2, 63, 64, 65, 130} x C in {1, 3, 64, 65, 130} x B in {1, 3}: the wave and
               lane tails, the channel tail, a partial last workgroup; and on the exact-operand cases.
  2 fixture    the device at the twin's bars: the reference's indices equal, values and gradients at 1e-5.
  3 module     losses.DescCGFLoss forward and loss.mean().backward() against the fixture and against the dense restatement
               in double from the recorded draws, at 1e-5 (inputs are float32: no gradcheck).
  4 graph      one call captured with the step as a device word, replayed twice with the word incremented in between: each
               replay equals an eager call at that step bit for bit, and the two replays select differently.
  5 launches   the launch log names the four kernels."""
import functools

import numpy as np
import pytest
import torch

import cgf_oracle as co
import test_cgf_loss_cpu as tc
from conftest import assert_close
from usip_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
MS, CS, BS = (1, 2, 63, 64, 65, 130), (1, 3, 64, 65, 130), (1, 3)


def dev(a):
    return tc.tens(a).to(DEV)


def run_device(c, grad=None, seed=0, step=0, elem_base=0):
    """tc.run_twin's counterpart on the device -> dict of numpy arrays"""
    t = {k: dev(c[k]) for k in tc.INPUTS}
    draws = None if c.get("u1") is None else {k: dev(c[k]) for k in ("u1", "u2", "u3")}
    sel, has, take_far = ops.cgf_select(t["anc_kp"], t["pos_kp"], float(c["radius"]), draws, seed, step, elem_base)
    loss, active, dist, coef = ops.cgf_loss(t["anc_desc"], t["pos_desc"], t["anc_sigma"], sel, has, take_far, float(c["gamma"]),
                                            float(c["sigma_max"]))
    g = dev(tc.grad_of(c) if grad is None else grad)
    d_anc, d_pos = ops.cgf_loss_backward(t["anc_desc"], t["pos_desc"], sel, take_far, dist, coef, g)
    return {k: v.cpu().numpy() for k, v in dict(sel=sel, has=has, take_far=take_far, loss=loss, active=active, dist=dist,
                                                coef=coef, d_anc=d_anc, d_pos=d_pos).items()}


@functools.lru_cache(maxsize=None)
def random_case(B, M, C, seed=0):
    """a mixed batch: near and far partners, some sigmas at or above sigma_max, one anchor descriptor equal to its partner's"""
    g = np.random.default_rng(1000 * M + C + seed)
    anc, pos = tc._cloud(M + 7 * C + seed, B, M)
    ad, pd = g.standard_normal((B, C, M)).astype(F), g.standard_normal((B, C, M)).astype(F)
    pd[:, :, 0] = ad[:, :, 0]
    u = lambda *s: (g.integers(0, 1 << 24, s).astype(F) * F(2.0 ** -24))      # noqa: E731   with exact zeros and ties
    return dict(anc_kp=anc, pos_kp=pos, anc_desc=ad, pos_desc=pd, anc_sigma=g.uniform(0, 1.3, (B, M)).astype(F), radius=1.0,
                gamma=0.5, sigma_max=1.0, u1=u(B, M, M), u2=u(B, M, M), u3=u(B, M), grad=g.standard_normal((B, M)).astype(F))


# ---------------------------------------------------------------------------------------------------- 1: the twin, bit for bit
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("M", MS)
def test_device_equals_the_twin_bit_for_bit(M, C):
    for B in BS:
        c = random_case(B, M, C)
        assert_same = functools.partial(tc.assert_same_bits, names=tc.OUTPUTS)
        assert_same(run_device(c, c["grad"]), tc.run_twin(c, 4, c["grad"]), tag="explicit B=%d M=%d C=%d" % (B, M, C))
        p = {k: v for k, v in c.items() if k not in ("u1", "u2", "u3")}
        assert_same(run_device(p, c["grad"], 5, 9, 3), tc.run_twin(p, 4, c["grad"], 5, 9, 3),
                    tag="philox B=%d M=%d C=%d" % (B, M, C))


@pytest.mark.parametrize("name", tc.EXACT)
def test_device_equals_the_twin_on_exact_operands(name):
    c = tc.exact_case(name)
    tc.assert_same_bits(run_device(c), tc.run_twin(c), tc.OUTPUTS, name)
    if name == "shared_neg":
        c = tc.exact_case(name, 130, 3)                                 # M terms in one column of d_pos
        tc.assert_same_bits(run_device(c), tc.run_twin(c), tc.OUTPUTS, name + " M=130")


def test_indices_read_from_memory_are_clamped_on_the_device():
    c = random_case(1, 2, 3)
    t = {k: dev(c[k]) for k in tc.INPUTS}
    sel = torch.tensor([[[7, -3, 99], [-1, 1 << 30, 5]]], dtype=torch.int32, device=DEV)
    has, tf = torch.ones((1, 2), dtype=torch.uint8, device=DEV), torch.tensor([[1, 0]], dtype=torch.uint8, device=DEV)
    clamped = torch.tensor([[[1, 0, 1], [0, 1, 1]]], dtype=torch.int32, device=DEV)
    a = ops.cgf_loss(t["anc_desc"], t["pos_desc"], t["anc_sigma"], sel, has, tf, 0.5, 1.0)
    b = ops.cgf_loss(t["anc_desc"], t["pos_desc"], t["anc_sigma"], clamped, has, tf, 0.5, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    g = dev(tc.grad_of(c))
    ga = ops.cgf_loss_backward(t["anc_desc"], t["pos_desc"], sel, tf, a[2], a[3], g)
    gb = ops.cgf_loss_backward(t["anc_desc"], t["pos_desc"], clamped, tf, a[2], a[3], g)
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))


# ---------------------------------------------------------------------------------------------------- 2: the reference fixture
@pytest.mark.parametrize("name", tc.CASES)
def test_device_matches_the_reference_fixture(name):
    c = tc.fixture(name)
    got = run_device(c)
    assert np.array_equal(got["sel"], c["sel"])
    assert np.array_equal(got["has"], c["has"]) and np.array_equal(got["take_far"], c["take_far"])
    assert_close(got["loss"], c["loss"], name=name + " loss")
    assert_close(got["active"], c["active"], name=name + " active")
    assert_close(got["d_anc"], c["d_anc"], name=name + " d_anc")
    assert_close(got["d_pos"], c["d_pos"], name=name + " d_pos")
    tc.assert_same_bits(got, tc.run_twin(c), tc.OUTPUTS, name)


# ---------------------------------------------------------------------------------------------------- 3: the module
@functools.lru_cache(maxsize=None)
def dense(name):
    """the dense double restatement on one fixture case -> (loss, active, d_anc, d_pos) as numpy; computed once"""
    c = tc.fixture(name)
    ad, pd = tc.tens(c["anc_desc"]).double().requires_grad_(True), tc.tens(c["pos_desc"]).double().requires_grad_(True)
    loss, active = co.dense_torch(tc.tens(c["anc_kp"]), ad, tc.tens(c["pos_kp"]), pd, tc.tens(c["anc_sigma"]).double(),
                                  float(c["radius"]), float(c["gamma"]), float(c["sigma_max"]), tc.tens(c["u1"]), tc.tens(c["u2"]),
                                  tc.tens(c["u3"]))
    loss.mean().backward()
    return loss.detach().numpy(), active.numpy(), ad.grad.numpy(), pd.grad.numpy()


@pytest.mark.parametrize("name", tc.CASES)
def test_module_forward_and_backward(name):
    from usip_amd.losses import DescCGFLoss
    c = tc.fixture(name)
    t = {k: dev(c[k]) for k in tc.INPUTS}
    t["anc_desc"].requires_grad_(True)
    t["pos_desc"].requires_grad_(True)
    mod = DescCGFLoss(tc.Opt(c)).to(DEV)
    draws = {k: dev(c[k]) for k in ("u1", "u2", "u3")}
    loss, active = mod(t["anc_kp"], t["anc_desc"], t["pos_kp"], t["pos_desc"], t["anc_sigma"], None, None, draws=draws)
    loss.mean().backward()
    assert loss.is_cuda and loss.shape == c["loss"].shape and active.shape == c["active"].shape
    assert np.array_equal(mod.last_indices[0].cpu().numpy(), c["sel"])
    got = (loss.detach().cpu().numpy(), active.cpu().numpy(), t["anc_desc"].grad.cpu().numpy(), t["pos_desc"].grad.cpu().numpy())
    for g, key, want in zip(got, ("loss", "active", "d_anc", "d_pos"), dense(name)):
        assert_close(g, c[key], name="%s %s against the fixture" % (name, key))
        assert_close(g, want, name="%s %s against the dense restatement" % (name, key))
    assert t["anc_kp"].grad is None and t["anc_sigma"].grad is None


def test_module_default_path_steps_a_device_counter():
    from usip_amd.losses import DescCGFLoss
    c = tc.fixture("batch3")
    t = [dev(c[k]) for k in ("anc_kp", "anc_desc", "pos_kp", "pos_desc", "anc_sigma")]
    mod = DescCGFLoss(tc.Opt(c), seed=3)
    mod(*t)
    a = [x.clone() for x in mod.last_indices]
    mod(*t)
    b = [x.clone() for x in mod.last_indices]
    assert not torch.equal(a[0], b[0]) and int(mod._step_dev.item()) == 2
    for step, got in ((0, a), (1, b)):                                  # the host twin draws the same numbers
        want = ops.cgf_select_cpu(t[0].cpu(), t[2].cpu(), float(c["radius"]), None, 3, step)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(got, want))
    mod.eval()
    mod(*t)
    assert int(mod._step_dev.item()) == 2


# ---------------------------------------------------------------------------------------------------- 4: graph capture
def test_a_captured_call_draws_anew_on_every_replay():
    from usip_amd.losses import DescCGFLoss
    c = random_case(3, 65, 65)
    t = {k: dev(c[k]) for k in tc.INPUTS}
    t["anc_desc"].requires_grad_(True)
    t["pos_desc"].requires_grad_(True)
    mod = DescCGFLoss(tc.Opt(c), seed=11)
    order = ("anc_kp", "anc_desc", "pos_kp", "pos_desc", "anc_sigma")

    def call(step):
        t["anc_desc"].grad = t["pos_desc"].grad = None
        loss, active = mod(*[t[k] for k in order], step=step)
        loss.mean().backward()
        return [loss.detach(), active, mod.last_indices[0], mod.last_indices[2], t["anc_desc"].grad, t["pos_desc"].grad]

    eager = {s: [x.clone() for x in call(s)] for s in (4, 5)}
    word = torch.full((1,), 4, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # the usual warm-up off the default stream
        call(word)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    t["anc_desc"].grad = t["pos_desc"].grad = None
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):    # one stream, no parallel branches
        held = call(word)
    seen = []
    for s in (4, 5):
        graph.replay()
        got = [x.clone() for x in held]
        for g, e in zip(got, eager[s]):
            assert g.dtype == e.dtype and torch.equal(g.view(torch.uint8), e.view(torch.uint8)), s
        seen.append(got[2])
        word.add_(1)
    assert not torch.equal(seen[0], seen[1])


# ---------------------------------------------------------------------------------------------------- 5: the launch log
def test_launch_log_names_the_kernels():
    lib = _lib.lib()
    c = random_case(1, 63, 3)
    lib.usip_launch_log(1)
    try:
        run_device(c)
        names = []
        while (name := lib.usip_launch_log_entry(len(names), None)) is not None:
            names.append(name.decode())
    finally:
        lib.usip_launch_log(0)
    assert len(names) == 4, names
    for n, want in zip(names, ("cgf_select_kernel", "cgf_dist_kernel", "cgf_row_kernel", "cgf_backward_kernel")):
        assert want in n, names
