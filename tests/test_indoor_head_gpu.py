"""DescriptorLiteOldGlobal / IndoorDescriptorStep on the device against the fixture captured from the reference
(tests/golden/indoor_head.npz, tests/golden/make_indoor_head_golden.py): ball indices and the loss's selection bit-exact;
descriptors (training and evaluation mode), active share, loss and BatchNorm buffers within 1e-5; every parameter gradient,
against the fixture's float32 one and against its float64 one, within max(1e-5, 2 x the reference's own float32 noise, stored
with the fixture) -- all at the reference's pool routes
and near-zero ReLU decisions and on its recorded draws, in the three fp32-accurate matmul modes.  Then the pool over the
keypoints on each dispatch path (M = 3, 64, 500, 512) against a float64 restatement of the head's tail, the step's bit
reproducibility eagerly and from a captured graph, and describe_keypoints."""
import numpy as np
import pytest
import torch

import indoor_oracle as io_
from conftest import assert_close, load_golden
from gemm_gpu_helpers import DEV, _logged

pytestmark = pytest.mark.gpu
KEYS = ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "anc_kp", "pos_kp", "anc_sigmas", "anc_R_pos", "anc_scale_pos", "anc_shift_pos")


def _options(g, **kw):
    from usip_amd.networks import IndoorOptions
    return IndoorOptions(descriptor_len=float(g["cfg_descriptor_len"]), ball_radius=float(g["cfg_ball_radius"]),
                         ball_nsamples=int(g["cfg_ball_nsamples"]), CGF_radius=float(g["cfg_CGF_radius"]),
                         triple_loss_gamma=float(g["cfg_triple_loss_gamma"]), sigma_max=float(g["cfg_sigma_max"]), **kw)


def _filled(g):
    from usip_amd import synth
    from usip_amd.networks import DescriptorLiteOldGlobal
    return synth.fill_parameters({k: tuple(v.shape) for k, v in DescriptorLiteOldGlobal(_options(g)).state_dict().items()})


def _batch(g, draws=True):
    from usip_amd.step import batch_to_device
    batch = batch_to_device(dict({k: g[k] for k in KEYS}, perm=g["perm"]), DEV)
    if draws:
        batch["draws"] = {k: torch.from_numpy(g[k]).to(DEV) for k in ("u1", "u2", "u3")}
    return batch


def _pins(g):
    B, C = g["idx/pool_arg_2"].shape
    pools = [torch.from_numpy(g["idx/pool_arg_%d" % i].astype(np.int64)) for i in range(3)]
    pools[2] = pools[2].reshape(B, C, 1)                         # the pool over the keypoints: one neighbourhood per cloud
    relu_fix = [(torch.from_numpy(g["idx/relu_near_idx_%d" % i].astype(np.int64)), torch.from_numpy(g["idx/relu_near_on_%d" % i]))
                for i in range(6)]
    return pools, relu_fix


def _graph_nodes(fn):
    seen, stack, names = set(), [fn], []
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        stack.extend(n for n, _ in f.next_functions)
    return names


def test_indoor_step_matches_the_reference(matmul_mode):
    from usip_amd import functional as Fh
    from usip_amd.step import IndoorDescriptorStep
    g = load_golden("indoor_head.npz")
    filled = _filled(g)
    st = IndoorDescriptorStep(_options(g), DEV)
    st.allow_pinned_decisions = True
    st.load_numpy_state(filled)
    # the forward's own decisions first: what does not depend on a near-tie is asserted, the floats are printed
    st.step(_batch(g))
    torch.cuda.synchronize()
    assert np.array_equal(st.descriptor.last_indices["ball_idx"].cpu().numpy(), g["idx/ball_idx"].astype(np.int32))
    sel, has, take_far = st.triplet_criteria.last_indices
    assert np.array_equal(sel.cpu().numpy(), g["idx/sel"])
    assert np.array_equal(has.cpu().numpy(), g["idx/has"]) and np.array_equal(take_far.cpu().numpy(), g["idx/take_far"])
    for k in ("descriptors", "triplet", "loss"):
        a, b = st.last[k].detach().cpu().numpy().astype(np.float64), g[k].astype(np.float64)
        print("unpinned %-12s %.2e" % (k, np.abs(a - b).max() / np.abs(b).max()))
    # ... then the reference's decisions pinned
    st = IndoorDescriptorStep(_options(g), DEV)
    st.allow_pinned_decisions = True
    st.load_numpy_state(filled)
    pools, relu_fix = _pins(g)
    with Fh.pinned_decisions(pools=[p.int() for p in pools], relu_fix=relu_fix) as pins:
        st.step(_batch(g))
    torch.cuda.synchronize()
    assert pins.leftover == (0, 0) and sum(pins.flips) <= 64, (pins.leftover, pins.flips)
    assert np.array_equal(st.descriptor.last_indices["ball_idx"].cpu().numpy(), g["idx/ball_idx"].astype(np.int32))
    sel, has, take_far = st.triplet_criteria.last_indices
    assert np.array_equal(sel.cpu().numpy(), g["idx/sel"])
    assert np.array_equal(has.cpu().numpy(), g["idx/has"]) and np.array_equal(take_far.cpu().numpy(), g["idx/take_far"])
    for k in ("descriptors", "active", "loss"):
        err = assert_close(st.last[k].detach().cpu().numpy(), g[k], name=k + " pinned")
        print("pinned %-12s %.2e" % (k, err))
    # (the single triplet terms are differences of two descriptor distances, a few times worse conditioned than the
    # descriptors they are taken from; the figure is printed, the bars are the descriptors', the loss's and the active share's)
    a, b = st.last["triplet"].detach().cpu().numpy().astype(np.float64), g["triplet"].astype(np.float64)
    print("pinned %-12s %.2e  (the reference's own float32 noise %.2e)" % ("triplet", np.abs(a - b).max() / np.abs(b).max(),
                                                                      float(g["noise/triplet"])))
    for k, v in st.descriptor.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert_close(v.cpu().numpy(), g["buf/" + k], name=k)
    biggest = max(float(v) for k, v in g.items() if k.startswith("grad_norm/"))
    bad, checked = {}, 0
    for k, p in st.descriptor.named_parameters():
        if float(g["grad_norm/" + k]) < 1e-5 * biggest:          # a conv bias in front of BatchNorm: analytically zero
            continue
        fix, tru = g["grad/" + k].ravel().astype(np.float64), g["grad64/" + k].ravel().astype(np.float64)
        hip = p.grad.detach().cpu().numpy().ravel().astype(np.float64)
        scale = max(np.abs(tru).max(), 1e-30)
        e = dict(hip_vs_fixture=np.abs(hip - fix).max() / scale, hip_vs_truth=np.abs(hip - tru).max() / scale)
        bar = max(1e-5, 2 * float(g["noise/" + k]))
        print("grad %-20s %s  bar %.2e" % (k, {n: "%.2e" % v for n, v in e.items()}, bar))
        checked += 1
        if not max(e.values()) <= bar:
            bad[k] = (e, bar)
    # evaluation mode, on the buffers the reference's step left
    st.descriptor.load_state_dict({k[len("buf/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("buf/")},
                                  strict=False)
    st.descriptor.eval()
    batch = _batch(g, draws=False)
    with torch.no_grad():
        desc, _ = st.descriptor(torch.cat((batch["anc_pc"], batch["pos_pc"])), torch.cat((batch["anc_sn"], batch["pos_sn"])),
                                torch.cat((batch["anc_kp"], batch["pos_kp"])), False, None, perm=batch["perm"])
    print("eval descriptors %.2e" % assert_close(desc.cpu().numpy(), g["descriptors_eval"], name="descriptors in evaluation mode"))
    assert checked == 21 and not bad, "gradients off with the decisions pinned: %s" % bad


class _pool_log:
    """every pooling launch of a block, as (neighbourhood size, neighbourhoods per cloud, kernel name)"""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        from usip_amd import _lib, ops
        self.saved = {n: getattr(ops, n) for n in ("group_max_wide", "group_max", "group_max_act")}
        for n, fn in self.saved.items():
            def logged(y4, *a, _fn=fn, **kw):
                out, got = _logged(_lib.lib(), lambda: _fn(y4, *a, **kw))
                self.calls.extend((int(y4.shape[3]), int(y4.shape[2]), k) for k, _ in got)
                return out
            setattr(ops, n, logged)
        return self

    def __exit__(self, *exc):
        from usip_amd import ops
        for n, fn in self.saved.items():
            setattr(ops, n, fn)
        return False


# M -> (functional._group_path(M), the kernel that pools the keypoints, fc1 in the row-bias form)
DISPATCH = {3: ("fallback", "::group_max_kernel<4>", False), 64: ("fused", "::group_max4_kernel<16, true>", True),
            500: ("fallback", "::group_max_kernel<64>", False), 512: ("wide", "::group_max_wide_kernel", True)}


@pytest.mark.parametrize("M", sorted(DISPATCH))
def test_the_pool_over_the_keypoints_on_each_dispatch_path(M):
    from usip_amd import functional as Fh
    from usip_amd import synth
    from usip_amd.networks import DescriptorLiteOldGlobal, IndoorOptions
    path, kernel, rowbias = DISPATCH[M]
    assert Fh._group_path(M) == path
    B, C, N, K = 2, 8, 64, 8
    rng = np.random.default_rng(M)
    net = DescriptorLiteOldGlobal(IndoorOptions(descriptor_len=C, ball_nsamples=K, ball_radius=0.3)).to(DEV)
    sd = net.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    net.load_state_dict({k: torch.as_tensor(v).reshape(sd[k].shape) for k, v in filled.items()})
    net.train()
    pc = torch.from_numpy(rng.uniform(-0.4, 0.4, (B, 3, N)).astype(np.float32)).to(DEV)
    sn = torch.from_numpy(rng.standard_normal((B, 4, N)).astype(np.float32)).to(DEV)
    kp = torch.from_numpy(rng.uniform(-0.4, 0.4, (B, 3, M)).astype(np.float32)).to(DEV)
    cot = torch.from_numpy(rng.standard_normal((B, C, M)).astype(np.float32)).to(DEV)
    kept = {}
    trunk = net._trunk

    def keeping(*a):
        d, xf = trunk(*a)
        d.retain_grad()
        kept["d"] = d
        return d, xf
    net._trunk = keeping
    with _pool_log() as log, Fh.pinned_decisions(record=True) as pins:
        out, _ = net(pc, sn, kp, True, None, perm=rng.permutation(N))
    names = _graph_nodes(out.grad_fn)
    out.backward(cot)
    torch.cuda.synchronize()
    # the pool is seen like any other: third in the record, one neighbourhood per cloud, the first arg-max
    d = kept["d"].detach()
    assert len(pins.pools) == 3 and tuple(pins.pools[2].shape) == (B, C, 1)
    assert torch.equal(pins.pools[2].long().squeeze(2), torch.max(d, dim=2)[1])
    mine = [k for size, groups, k in log.calls if (size, groups) == (M, 1)]
    assert len(mine) == 1 and kernel in mine[0], (kernel, log.calls)
    # fc1 in the row-bias form has no concatenated tensor; the literal form has
    assert any(n.startswith("CatBackward") for n in names) == (not rowbias), names
    assert sum("SharedMLPLayerPooled" in n for n in names) == (2 if rowbias else 1), names
    # the tail against the float64 restatement, at the bar the float32 restatement's own error sets
    spread = []

    def tail(dtype):
        leaf = d.cpu().to(dtype).requires_grad_(True)
        P = {k: v.detach().cpu().to(dtype).requires_grad_(v.dtype.is_floating_point and "running" not in k)
             for k, v in net.state_dict().items() if k.startswith("fc")}
        o = io_.head_tail(leaf, P, training=True, spread=spread if dtype == torch.float64 else None)
        o.backward(cot.cpu().to(dtype))
        grads = {k: v.grad for k, v in P.items() if v.requires_grad and v.grad is not None}
        grads["d"] = leaf.grad
        return o.detach(), grads
    o64, g64 = tail(torch.float64)
    o32, g32 = tail(torch.float32)
    print("M=%d descriptor err %.2e  float32 restatement %.2e  mean^2 / variance of fc1, fc2: %s" % (
        M, float((out.detach().cpu().double() - o64).abs().max() / o64.abs().max()),
        float((o32.double() - o64).abs().max() / o64.abs().max()), ["%.1f" % v for v in spread]))
    assert_close(out.detach().cpu().numpy(), o64.numpy(), name="descriptor M=%d" % M)
    mine = {k: p.grad.detach().cpu() for k, p in net.named_parameters() if k.startswith("fc")}
    mine["d"] = kept["d"].grad.detach().cpu()
    bad = {}
    for k, t64 in g64.items():
        if k.endswith("conv.bias") and not k.startswith("fc3"):
            continue                                             # in front of BatchNorm: analytically zero
        scale = max(float(t64.abs().max()), 1e-30)
        noise = float((g32[k].double() - t64).abs().max()) / scale
        err = float((mine[k].double() - t64).abs().max()) / scale
        print("M=%d %-18s err %.2e  float32 restatement %.2e" % (M, k, err, noise))
        if not err <= max(1e-5, 2 * noise):
            bad[k] = (err, noise)
    assert not bad, bad


def _two_steps(graph, calls, g, filled):
    from usip_amd.step import IndoorDescriptorStep
    st = IndoorDescriptorStep(_options(g), DEV, with_optimizer=True, graph=graph, seed=7)
    st.load_numpy_state(filled)
    batch = _batch(g, draws=False)
    out = []
    for _ in range(calls):
        loss = st.step(batch).detach().clone()
        torch.cuda.synchronize()
        out.append((loss, st.last["descriptors"].detach().clone(), st.last["triplet"].detach().clone(),
                    st.bucket.flat_param.data.clone(), st.triplet_criteria.last_indices[0].clone()))
    return st, out


def test_the_step_reproduces_its_bits_eagerly_and_from_a_captured_graph():
    g = load_golden("indoor_head.npz")
    filled = _filled(g)
    _, a = _two_steps(False, 4, g, filled)
    _, b = _two_steps(False, 4, g, filled)
    st, c = _two_steps(True, 4, g, filled)                       # two eager calls, the capture and its replay, a replay
    assert st.use_graph and len(st._graphs) == 1
    for i in range(4):
        for x, y, z in zip(a[i], b[i], c[i]):
            assert torch.equal(x, y), ("eager", i)
            assert torch.equal(x, z), ("graph", i)
    assert not torch.equal(a[0][3], a[1][3])                     # Adam moved the parameters ...
    assert not all(torch.equal(a[i][4], a[i + 1][4]) for i in range(3))   # ... and every call drew anew, replays included


def test_the_dropout_option_raises_and_test_model_runs():
    from usip_amd.step import IndoorDescriptorStep
    g = load_golden("indoor_head.npz")
    with pytest.raises(NotImplementedError, match="random_pc_dropout_lower_limit"):
        IndoorDescriptorStep(_options(g, random_pc_dropout_lower_limit=0.5), DEV)
    st = IndoorDescriptorStep(_options(g), DEV)
    st.load_numpy_state(_filled(g))
    st.descriptor.load_state_dict({k[len("buf/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("buf/")},
                                  strict=False)
    before = {k: v.clone() for k, v in st.descriptor.state_dict().items()}
    loss = st.test_model(_batch(g))
    assert torch.isfinite(loss) and not loss.requires_grad
    assert_close(st.last["descriptors"].cpu().numpy(), g["descriptors_eval"], name="test_model descriptors")
    assert all(torch.equal(v, before[k]) for k, v in st.descriptor.state_dict().items())   # evaluation mode moves nothing


def test_describe_keypoints_takes_the_head_as_it_is():
    from usip_amd import inference
    from usip_amd.networks import DescriptorLiteOldGlobal
    g = load_golden("indoor_head.npz")
    net = DescriptorLiteOldGlobal(_options(g)).to(DEV)
    sd = net.state_dict()
    net.load_state_dict({k: torch.as_tensor(v).reshape(sd[k].shape) for k, v in _filled(g).items()})
    b = _batch(g, draws=False)
    desc = inference.describe_keypoints(net, b["anc_pc"], b["anc_sn"], b["anc_kp"])
    assert tuple(desc.shape) == (2, 64, 24) and not net.training
    assert float((torch.norm(desc.double(), dim=1) - 1).abs().max()) < 1e-4
    assert torch.equal(desc, inference.describe_keypoints(net, b["anc_pc"], b["anc_sn"], b["anc_kp"]))
