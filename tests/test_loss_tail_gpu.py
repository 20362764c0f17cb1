"""csrc/loss_tail.hip: the detector step's loss segment in three launches and one backward launch.

Every comparison is bit for bit (the int32 view of every float tensor, torch.equal) against the chain of launches the
step ran before and still runs with ops.LOSS_TAIL off -- rigid_transform, nearest in both directions, chamfer_prob, the
keypoint-on-cloud nearest, detector_loss_combine, and autograd through them -- on the same inputs: the six scalars,
kp_t, (a, J), (c, I) forward; the gradients of keypoints and sigmas for an upstream gradient of 1.0 and of 0.375."""
import ctypes

import numpy as np
import pytest
import torch

from test_segment_kernels_gpu import _launched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
ALPHA = 0.7
GLOSS = (1.0, 0.375)
SHAPES = [(1, 1), (1, 3), (2, 64), (3, 65), (2, 512), (1, 1023), (1, 1024)]
QUARTER = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)        # a rotation that is exact in float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _inputs(B, M, N, seed, kind="random"):
    """-> numpy (kp [2B,3,M], sg [2B,M], R [B,3,3], scale [B], shift [B,3], pc [2B,3,N])."""
    from usip_amd import synth
    rng = np.random.default_rng(seed)
    pc = np.stack([synth.make_cloud(rng, N, "slab:12") for _ in range(2 * B)]).astype(F)
    pick = rng.integers(0, N, (2 * B, M))
    kp = np.stack([pc[b][:, pick[b]] for b in range(2 * B)]) + rng.normal(0, 0.3, (2 * B, 3, M))
    kp = kp.astype(F)
    sg = rng.uniform(0.2, 3.0, (2 * B, M)).astype(F)
    R = np.stack([_rotation(rng) for _ in range(B)])
    scale = rng.uniform(0.6, 1.6, B)
    shift = rng.normal(0, 1.0, (B, 3))
    if kind in ("equal", "duplicates"):
        # dyadic src keypoints, a quarter turn, scale 2, dyadic shift: t is exact, and dst is set to exactly t
        src = np.round(rng.uniform(-8, 8, (B, 3, M)) * 16) / 16
        if kind == "duplicates" and M > 5:
            src[:, :, 5] = src[:, :, 2]                       # t_5 == t_2 == q_2 == q_5: the first index wins
            src[:, :, M - 1] = src[:, :, 0]
        R = np.stack([QUARTER] * B)
        scale = np.full(B, 2.0)
        shift = np.round(rng.uniform(-4, 4, (B, 3)) * 8) / 8
        dst = 2.0 * np.einsum("bij,bjm->bim", R, src) + shift[:, :, None]
        kp = np.concatenate((src, dst)).astype(F)
        assert np.array_equal(kp[:B].astype(np.float64), src) and np.array_equal(kp[B:].astype(np.float64), dst)
    elif kind == "one_partner":
        # every transformed src keypoint lies within 0.5 of dst keypoint 0; the other dst keypoints are 100 away
        t = rng.uniform(-0.25, 0.25, (B, 3, M))
        src = np.einsum("bji,bjm->bim", R, t - shift[:, :, None]) / scale[:, None, None]
        dst = rng.uniform(-0.25, 0.25, (B, 3, M)) + 100.0
        dst[:, :, 0] = 0.0
        kp = np.concatenate((src, dst)).astype(F)
    elif kind == "sigmas":
        sg = (10.0 ** rng.uniform(-3, 3, (2 * B, M))).astype(F)
        sg.reshape(-1)[:2] = (1e-3, 1e3)
    return kp, sg, R.astype(F), scale.astype(F), shift.astype(F), pc


def _grid(pc):
    from usip_amd import ops
    return ops.cell_grid_build(pc, 2.0625)


def _chain(kp, sg, R, scale, shift, pc, grid):
    """The step's chain (usip_amd/step.py, ops.LOSS_TAIL off) -> dict of results and gradients."""
    from usip_amd import functional as Fh
    kp, sg = kp.clone().requires_grad_(True), sg.clone().requires_grad_(True)
    B = kp.shape[0] // 2
    kp_src, kp_dst = torch.split(kp, B, dim=0)
    sg_src, sg_dst = torch.split(sg, B, dim=0)
    kp_t = Fh.rigid_transform(kp_src, R, scale, shift)
    a, J = Fh.nearest_distance_i32(kp_t, kp_dst)
    c, I = Fh.nearest_distance_i32(kp_dst, kp_t)
    loss_chamfer, pure, weighted = Fh.chamfer_prob(a, J, c, I, sg_src, sg_dst)
    d, _ = Fh.nearest_distance_i32(kp, pc, grid)
    loss, on_src, on_dst = Fh.detector_loss_combine(d, loss_chamfer, ALPHA)
    out = dict(loss=loss, loss_chamfer=loss_chamfer, pure=pure, weighted=weighted, on_src=on_src, on_dst=on_dst,
               kp_t=kp_t, a=a, J=J, c=c, I=I)
    for g in GLOSS:
        out["g_kp", g], out["g_sg", g] = torch.autograd.grad(loss, (kp, sg), torch.tensor(g, device=DEV),
                                                             retain_graph=True)
    return {k: v.detach() for k, v in out.items()}


def _fused(kp, sg, R, scale, shift, pc, grid):
    from usip_amd import functional as Fh, ops
    kp, sg = kp.clone().requires_grad_(True), sg.clone().requires_grad_(True)
    loss, loss_chamfer, pure, weighted, on_src, on_dst, J, I = Fh.detector_loss_tail(kp, sg, R, scale, shift, pc, grid,
                                                                                     ALPHA)
    kp_t, a, J2, c, I2 = ops.loss_tail_scan(kp.detach(), R, scale, shift)
    assert torch.equal(J, J2) and torch.equal(I, I2)
    out = dict(loss=loss, loss_chamfer=loss_chamfer, pure=pure, weighted=weighted, on_src=on_src, on_dst=on_dst,
               kp_t=kp_t, a=a, J=J, c=c, I=I)
    for g in GLOSS:
        out["g_kp", g], out["g_sg", g] = torch.autograd.grad(loss, (kp, sg), torch.tensor(g, device=DEV),
                                                             retain_graph=True)
    return {k: v.detach() for k, v in out.items()}


def _compare(B, M, N, seed, kind, with_grid):
    t = [_dev(x) for x in _inputs(B, M, N, seed, kind)]
    grid = _grid(t[5]) if with_grid else None
    want, got = _chain(*t, grid), _fused(*t, grid)
    assert want.keys() == got.keys()
    for k in want:
        assert _same(want[k], got[k]), (k, (want[k] != got[k]).nonzero()[:4].tolist())
    return t, want


@pytest.mark.parametrize("with_grid", (False, True), ids=("scan", "grid"))
@pytest.mark.parametrize("N", (256, 2048))
@pytest.mark.parametrize("B,M", SHAPES)
def test_fused_segment_equals_the_chain_on_random_keypoints(B, M, N, with_grid):
    t, want = _compare(B, M, N, 1000 * B + M + N, "random", with_grid)
    assert bool((want["a"] > 0).all()) and bool(torch.isfinite(want["g_kp", 1.0]).all())
    if M >= 64:                                               # a real rotation and scale, several sources per partner
        assert not _same(want["kp_t"], t[0][:B]) and int(torch.bincount(want["J"].reshape(-1).long()).max()) > 1


@pytest.mark.parametrize("B,M", [(2, 64), (3, 65), (1, 1024)])
def test_src_set_equal_to_the_dst_set_after_the_transform(B, M):
    _, want = _compare(B, M, 256, 7 + M, "equal", True)
    assert not want["a"].any() and not want["c"].any()       # every distance is exactly zero
    assert bool(want["g_sg", 1.0].ne(0).all())                # the sigmas still receive their 1 / s


@pytest.mark.parametrize("B,M", [(2, 64), (3, 65)])
def test_duplicated_keypoints_take_the_first_index_and_no_gradient(B, M):
    from usip_amd import functional as Fh
    t, want = _compare(B, M, 256, 11 + M, "duplicates", True)
    assert not want["a"].any() and not want["c"].any()
    # at zero distance the chamfer term sends nothing to the keypoints: their gradient is the on-cloud term's alone
    kp = t[0].clone().requires_grad_(True)
    d, _ = Fh.nearest_distance_i32(kp, t[5])
    (on_cloud,) = torch.autograd.grad(Fh.detector_loss_combine(d, torch.zeros(1, device=DEV), ALPHA)[0], kp)
    assert torch.equal(on_cloud, want["g_kp", 1.0]) and bool(on_cloud.ne(0).any())
    J, I = want["J"].cpu().numpy(), want["I"].cpu().numpy()
    assert (J[:, 5] == 2).all() and (I[:, 5] == 2).all() and (J[:, M - 1] == 0).all() and (I[:, M - 1] == 0).all()
    assert (J[:, 2] == 2).all() and (J[:, 0] == 0).all()


@pytest.mark.parametrize("B,M", [(2, 64), (3, 65), (1, 1023)])
def test_all_src_keypoints_share_one_partner(B, M):
    _, want = _compare(B, M, 256, 13 + M, "one_partner", False)
    assert not want["J"].any()                                # dst keypoint 0 has M contributions, the others none
    g = want["g_kp", 1.0]
    assert bool(g[B:, :, 0].ne(0).any())


@pytest.mark.parametrize("B,M", [(2, 64), (3, 65), (2, 512)])
def test_sigmas_over_six_decades(B, M):
    t, want = _compare(B, M, 256, 17 + M, "sigmas", True)
    assert float(t[1].min()) <= F(1e-3) and float(t[1].max()) >= F(1e3)
    assert bool(torch.isfinite(want["loss"])) and bool(torch.isfinite(want["g_sg", 0.375]).all())


def test_launches_of_one_fused_forward_and_backward():
    """Forward: scan, the on-cloud search through the grid, sums.  Backward: one launch, and the autograd graph holds
    nothing else between the loss and the two inputs (no split, no gradient sum)."""
    from usip_amd import functional as Fh, ops
    B, M = 2, 64
    kp, sg, R, scale, shift, pc = [_dev(x) for x in _inputs(B, M, 2048, 3)]
    grid = _grid(pc)
    kp.requires_grad_(True)
    sg.requires_grad_(True)
    out, log = _launched(lambda: Fh.detector_loss_tail(kp, sg, R, scale, shift, pc, grid, ALPHA))
    assert [n for n, _ in log] == ["loss_tail_scan_kernel", "nearest_grid_kernel", "loss_tail_sums_kernel"], log
    assert log[0][1] == 4 * B and log[2][1] == 1
    loss = out[0]
    assert type(loss.grad_fn).__name__ == "_DetectorLossTailBackward"
    nxt = [type(f).__name__ for f, _ in loss.grad_fn.next_functions if f is not None]
    assert nxt == ["AccumulateGrad", "AccumulateGrad"], nxt
    assert all(not o.requires_grad for o in out[1:])
    g_kp, g_sg = torch.autograd.grad(loss, (kp, sg), torch.tensor(0.375, device=DEV))
    # the launch log belongs to the calling thread and autograd runs device work on its own: the same call, made here
    kp_t, a, J, c, I = ops.loss_tail_scan(kp.detach(), R, scale, shift)
    d, arg = ops.nearest_grid(kp.detach(), grid)
    (w_kp, w_sg), log = _launched(lambda: ops.loss_tail_backward(
        torch.tensor([0.375], device=DEV), kp.detach(), sg.detach(), kp_t, a, J, c, I, d, arg, pc, R, scale,
        ALPHA / (B * M)))
    assert log == [("loss_tail_bwd_kernel", B)], log
    assert _same(g_kp, w_kp) and _same(g_sg, w_sg)


def test_entries_refuse_what_they_cannot_stage():
    """M = 0, M = 1025 and a null pointer: non-zero, nothing launched, outputs untouched."""
    from usip_amd import _lib
    lib = _lib.lib()
    B, M, N = 1, 8, 16
    f = lambda *s: torch.full(s, -7.0, device=DEV)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    kp, sg, kp_t, a, c, d, pc = f(2 * B, 3, 1025), f(2 * B, 1025), f(B, 3, 1025), f(B, 1025), f(B, 1025), f(2 * B, 1025), f(2 * B, 3, N)
    J, I, arg = i(B, 1025), i(B, 1025), i(2 * B, 1025)
    R, scale, shift, out6, gloss = f(B, 9), f(B), f(B, 3), f(6), f(1)
    g_kp, g_sg = f(2 * B, 3, 1025), f(2 * B, 1025)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def scan(m, kp_ptr):
        return lib.usip_loss_tail_scan_f32(kp_ptr, p(R), p(scale), p(shift), p(kp_t), p(a), p(J), p(c), p(I), B, m, None)

    def sums(m, a_ptr):
        return lib.usip_loss_tail_sums_f32(a_ptr, p(J), p(c), p(I), p(sg), p(d), 0.5, p(out6), B, m, None)

    def bwd(m, g_ptr):
        return lib.usip_loss_tail_backward_f32(g_ptr, p(kp), p(sg), p(kp_t), p(a), p(J), p(c), p(I), p(d), p(arg),
                                               p(pc), p(R), p(scale), 0.5, p(g_kp), p(g_sg), B, m, N, None)

    for call, first in ((scan, kp), (sums, a), (bwd, gloss)):
        for m, ptr in ((0, p(first)), (1025, p(first)), (M, None)):
            rc, log = _launched(lambda: call(m, ptr))
            assert rc != 0 and log == [], (call.__name__, m, rc, log)
    torch.cuda.synchronize()
    for t in (kp_t, a, c, out6, g_kp, g_sg):
        assert bool((t == -7.0).all())
    assert bool((J == -7).all()) and bool((I == -7).all())
    rc, log = _launched(lambda: lib.usip_loss_tail_scan_f32(p(kp), p(R), p(scale), p(shift), p(kp_t), p(a), p(J), p(c),
                                                             p(I), 65536, M, None))
    assert rc != 0 and log == []


def test_python_keeps_the_chain_where_the_fused_entries_do_not_apply(monkeypatch):
    from usip_amd import functional as Fh, ops
    kp, sg = torch.zeros(4, 3, 1025, device=DEV), torch.zeros(4, 1025, device=DEV)
    assert not Fh.detector_loss_tail_supported(kp, sg)
    assert Fh.detector_loss_tail_supported(kp[:, :, :1024], sg[:, :1024])
    assert not Fh.detector_loss_tail_supported(kp[:, :, :64].cpu(), sg[:, :64].cpu())
    assert not Fh.detector_loss_tail_supported(kp[:, :, :64], None)
    monkeypatch.setattr(ops, "LOSS_TAIL", False)
    assert not Fh.detector_loss_tail_supported(kp[:, :, :64], sg[:, :64])


def test_detector_step_is_the_same_with_and_without_the_fused_segment(monkeypatch):
    """DetectorStep("ball") with ops.LOSS_TAIL on and off (what USIP_LOSS_TAIL=0 sets when the package is imported):
    eager, then graph replay, five batches with Adam.  Every tensor of st.last, every index tensor and every parameter
    must be equal bit for bit; forward_losses alone (no backward) gives the same loss either way."""
    from usip_amd import ops, synth
    from usip_amd.networks import DetectorOptions
    from usip_amd.step import DetectorStep, batch_to_device
    opt = DetectorOptions(surface_normal_len=4, node_knn_k_1=8)
    batches = [batch_to_device(synth.make_pair_batch(60 + i, 2, 2048, 64, 4, "slab:14"), DEV) for i in range(5)]

    def run(flag, graph):
        monkeypatch.setattr(ops, "LOSS_TAIL", flag)
        torch.manual_seed(9)
        st = DetectorStep("ball", opt, DEV, with_optimizer=True, graph=graph)
        seen = []
        for n, b in enumerate(batches):                # graph: calls 1-2 eager, 3 captures and replays, 4-5 replay
            st.step(b)
            if n == 0:
                fused = type(st.last["loss"].grad_fn).__name__ == "_DetectorLossTailBackward"
                assert fused == flag
            J, I = st.chamfer_criteria.last_indices
            seen.append({k: v.detach().clone() for k, v in list(st.last.items()) + list(st.detector.last_indices.items())
                         + [("chamfer_J", J), ("chamfer_I", I)]})
        return seen, {k: v.detach().clone() for k, v in st.detector.state_dict().items()}, st

    for graph in (False, True):
        (on, p_on, st_on), (off, p_off, st_off) = run(True, graph), run(False, graph)
        for i, (a, b) in enumerate(zip(on, off)):
            assert a.keys() == b.keys()
            for k in a:
                assert _same(a[k], b[k]), (graph, i, k)
        for k in p_on:
            assert _same(p_on[k], p_off[k]), (graph, k)
        if not graph:
            monkeypatch.setattr(ops, "LOSS_TAIL", True)
            l_on = st_on.forward_losses(st_on._prepare(batches[0])).detach().clone()
            monkeypatch.setattr(ops, "LOSS_TAIL", False)
            l_off = st_off.forward_losses(st_off._prepare(batches[0])).detach().clone()
            assert _same(l_on, l_off)
