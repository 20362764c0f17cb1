"""DescriptorLiteOld / DescriptorStep at the indoor neighbourhood size, ball_nsamples = 448, against the fixture captured from the
reference (tests/golden/descriptor_wide_ball.npz, tests/golden/make_wide_ball_golden.py): one truncated and several padded balls.
Once on the wide kernels (csrc/group_wide.hip: one pooling pass over the pre-BN output, the row-bias form of conv4, per-
neighbourhood sums from the reduction pass) and once with ops.WIDE_GROUPS off (the activated tensor materialised, the literal
concat), in all three fp32-accurate matmul modes.  Ball indices bit-exact; descriptors, loss and every parameter gradient within
1e-5, the gradients at pinned pool and near-zero ReLU decisions as tests/test_modules_gpu.py does for descriptor_micro."""
import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden
from gemm_gpu_helpers import DEV, _logged

pytestmark = pytest.mark.gpu
KEYS = ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "anc_kp", "pos_kp", "anc_sigmas", "neg_idx")


def _options(g):
    from usip_amd.networks import DetectorOptions
    return DetectorOptions(surface_normal_len=4, descriptor_len=int(g["cfg_descriptor_len"]),
                           ball_radius=float(g["cfg_ball_radius"]), ball_nsamples=int(g["cfg_ball_nsamples"]))


class _wide:
    """`with _wide(on):` -- ops.WIDE_GROUPS for one block; .names: every kernel the wide and the narrow pooling / reduction
    wrappers launched meanwhile (the launch log holds eight entries, a step launches more: each call is logged by itself)"""

    def __init__(self, on):
        self.on, self.names = bool(on), []

    def __enter__(self):
        from usip_amd import _lib, ops
        self.prev = ops.WIDE_GROUPS
        ops.WIDE_GROUPS = self.on
        self.saved = {n: getattr(ops, n) for n in ("group_max_wide", "bn_backward_reduce_wide", "group_max", "bn_backward_reduce")}
        for n, fn in self.saved.items():
            def logged(*a, _fn=fn, **kw):
                out, got = _logged(_lib.lib(), lambda: _fn(*a, **kw))
                self.names.extend(k for k, _ in got)
                return out
            setattr(ops, n, logged)
        return self

    def __exit__(self, *exc):
        from usip_amd import ops
        ops.WIDE_GROUPS = self.prev
        for n, fn in self.saved.items():
            setattr(ops, n, fn)
        return False


def _step(g, filled, pins=None):
    from usip_amd import functional as Fh
    from usip_amd.step import DescriptorStep, batch_to_device
    st = DescriptorStep(_options(g), DEV)
    st.allow_pinned_decisions = True
    st.load_numpy_state(filled)
    st.descriptor.fixed_permutation = g["perm"]
    batch = batch_to_device({k: g[k] for k in KEYS}, DEV)
    if pins is None:
        st.step(batch)
        used = None
    else:
        with Fh.pinned_decisions(pools=[p.int() for p in pins[0]], relu_fix=pins[1]) as used:
            st.step(batch)
    torch.cuda.synchronize()
    return st, used


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


def test_wide_descriptor_step_matches_the_reference(matmul_mode):
    from oracle import detector as od
    from usip_amd import synth
    from usip_amd.networks import DescriptorLiteOld
    g = load_golden("descriptor_wide_ball.npz")
    K, radius = int(g["cfg_ball_nsamples"]), float(g["cfg_ball_radius"])
    assert K == 448 and (g["ball_members"] >= K).any() and ((g["ball_members"] > 0) & (g["ball_members"] < K)).any()
    shapes = {k: tuple(v.shape) for k, v in DescriptorLiteOld(_options(g)).state_dict().items()}
    filled = synth.fill_parameters(shapes)
    n_pools = sum(k.startswith("idx/pool_arg_") for k in g)
    n_relu = sum(k.startswith("idx/relu_near_idx_") for k in g)
    assert (n_pools, n_relu) == (2, 4)
    pools = [torch.from_numpy(g["idx/pool_arg_%d" % i].astype(np.int64)) for i in range(n_pools)]
    relu_fix = [(torch.from_numpy(g["idx/relu_near_idx_%d" % i].astype(np.int64)), torch.from_numpy(g["idx/relu_near_on_%d" % i]))
                for i in range(n_relu)]

    def oracle(dtype, tape):
        P = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in filled.items()
             if not ("running_" in k or "num_batches" in k)}
        bufs = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in filled.items() if "running_" in k}
        batch = {k: torch.from_numpy(g[k]) for k in KEYS}
        batch = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in batch.items()}
        od.TAPE = tape
        try:
            res = od.descriptor_step(P, bufs, batch, torch.from_numpy(g["perm"]), radius=radius, K=K)
        finally:
            od.TAPE = None
        return P, res

    tape = od.DecisionTape(pools=pools, relu_fix=relu_fix)
    ref32, res32 = oracle(torch.float32, tape)
    assert tape.pools == [] and tape.relu_fix == []
    truth, _ = oracle(torch.float64, od.DecisionTape(replay=tape.rec))
    assert np.array_equal(res32["ball_idx"].numpy(), g["idx/ball_idx"].astype(np.int64))      # the oracle's query is the fixture's
    grads = {}
    for on in (True, False):
        # the forward's own decisions first: ball indices bit-exact, floats at the project's bar
        with _wide(on) as w:
            st, _ = _step(g, filled)
        assert np.array_equal(st.descriptor.last_indices["ball_idx"].cpu().numpy(), g["idx/ball_idx"].astype(np.int32))
        for k in ("descriptors", "triplet", "active", "loss"):
            assert_close(st.last[k].detach().cpu().numpy(), g[k], name="%s wide=%d" % (k, on))
        for k, v in st.descriptor.state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                assert_close(v.cpu().numpy(), g["buf/" + k], name=k)
        wide = [n for n in w.names if "group_max_wide_kernel" in n or "bn_bwd_reduce_wide_kernel" in n]
        if on:
            assert any("group_max_wide_kernel" in n for n in wide) and any("bn_bwd_reduce_wide_kernel" in n for n in wide), w.names
            assert not any("::group_max_kernel<" in n or "::bn_bwd_reduce_kernel<true" in n for n in w.names), w.names
        else:
            assert not wide and any("::group_max_kernel<64>" in n for n in w.names), w.names
        # ... then the reference's decisions pinned: every parameter gradient, entry by entry
        with _wide(on):
            st, pins = _step(g, filled, (pools, relu_fix))
        assert pins.leftover == (0, 0) and sum(pins.flips) <= 64
        for k in ("descriptors", "triplet", "active", "loss"):
            assert_close(st.last[k].detach().cpu().numpy(), g[k], name="%s pinned wide=%d" % (k, on))
        j_pos, j_neg = st.triplet_criteria.last_indices
        assert np.array_equal(j_pos.cpu().numpy(), res32["nn_pos"].numpy())
        assert np.array_equal(j_neg.cpu().numpy(), res32["nn_neg"].numpy())
        biggest = max(float(v) for k, v in g.items() if k.startswith("grad_norm/"))
        bad = {}
        grads[on] = {}
        for k, p in st.descriptor.named_parameters():
            gn = float(g["grad_norm/" + k])
            if gn < 1e-5 * biggest:
                continue
            hip = p.grad.detach().cpu().numpy().ravel().astype(np.float64)
            grads[on][k] = hip
            r32 = ref32[k].grad.numpy().ravel().astype(np.float64)
            tru = truth[k].grad.numpy().ravel()
            fix = g["grad/" + k].ravel().astype(np.float64)
            scale = max(np.abs(tru).max(), 1e-30)
            ref_noise = np.abs(r32 - tru).max() / scale
            bar = max(1e-5, 2 * ref_noise)
            e = dict(hip_vs_ref32=np.abs(hip - r32).max() / scale, hip_vs_truth=np.abs(hip - tru).max() / scale,
                     hip_vs_fixture=np.abs(hip - fix).max() / scale, ref32_vs_truth=ref_noise)
            print("grad %-24s wide=%d %s" % (k, on, {a: "%.2e" % b for a, b in e.items()}))
            if max(e["hip_vs_ref32"], e["hip_vs_truth"], e["hip_vs_fixture"]) > bar:
                bad[k] = e
        assert not bad, "descriptor gradients off with the decisions pinned (wide=%d): %s" % (on, bad)
    for k in grads[True]:                                       # the two paths agree with each other
        scale = max(np.abs(grads[False][k]).max(), 1e-30)
        assert np.abs(grads[True][k] - grads[False][k]).max() / scale <= 1e-5, k


def test_the_wide_path_builds_no_concat_in_front_of_conv4():
    """The autograd graph of the forward: on the wide kernels no CatBackward node at all (conv4 takes h and the pooled feature
    apart: the row-bias form); with WIDE_GROUPS off the literal cat(h, expand(pooled)) is there."""
    from usip_amd import synth
    from usip_amd.step import DescriptorStep, batch_to_device
    g = load_golden("descriptor_wide_ball.npz")
    for on in (True, False):
        with _wide(on):
            st = DescriptorStep(_options(g), DEV)
            st.load_numpy_state(synth.fill_parameters({k: tuple(v.shape) for k, v in st.descriptor.state_dict().items()}))
            st.descriptor.fixed_permutation = g["perm"]
            loss = st.forward_losses(st._prepare(batch_to_device({k: g[k] for k in KEYS}, DEV)))
            names = _graph_nodes(loss.grad_fn)
        assert any("SharedMLPLayerPooled" in n for n in names) == on, names
        assert any(n.startswith("CatBackward") for n in names) == (not on), names


def test_a_captured_wide_step_replays_the_eager_bits():
    from usip_amd import synth
    from usip_amd.step import DescriptorStep, batch_to_device
    g = load_golden("descriptor_wide_ball.npz")
    torch.manual_seed(4)
    eager = DescriptorStep(_options(g), DEV)
    graph = DescriptorStep(_options(g), DEV, graph=True)
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in eager.descriptor.state_dict().items()})
    eager.load_numpy_state(filled)
    graph.load_numpy_state(filled)
    batch = batch_to_device(dict({k: g[k] for k in KEYS}, perm=g["perm"]), DEV)
    le = eager.step(batch).detach().clone()
    want = (le, eager.last["descriptors"].detach().clone(), eager.bucket.flat.clone())
    for i in range(4):                                          # two eager calls, the capture, then replays
        lg = graph.step(batch).detach()
        torch.cuda.synchronize()
        assert torch.equal(lg, want[0]), i
        assert torch.equal(graph.last["descriptors"].detach(), want[1]), i
        assert torch.equal(graph.bucket.flat, want[2]), i
    assert graph.use_graph and len(graph._graphs) == 1
