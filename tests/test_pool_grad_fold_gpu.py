"""The gradient of a layer output that is max-pooled AND passed on (functional.group_max_fork: models/networks.py:706-709,
layers.py:433-436) used to be completed by a pass of its own over the dense gradient, dz[row][arg[row]] += dpooled[row]
(csrc/group.hip).  The GEMM that PRODUCES the dense gradient in the KNN fusion module now adds the pooling part at its store
where it can (FORK: csrc/gemm_x2f.hip); USIP_POOL_GRAD_FOLD=0 / ops.POOL_GRAD_FOLD = False keeps the stand-alone pass.

What must hold: the folded dX is BIT-equal to "unfused kernel, then group_max_backward_add_" (the same single fp32 add on
the same value), so the whole step is bit-equal with and without the fold, and every launch the guards refuse runs the old
path.  (The fused 64 -> 128 layer backward of the Ball front end does NOT take the fold: its BatchNorm-backward sums would run
over dense + sparse in one fp32 chain, which moves conv1-conv3's gradients at rounding level and, through Adam, a training
run; that site keeps its stand-alone pass.)"""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _launched(lib, call):
    """-> (call(), the demangled names of the kernels the library launched for it on this thread, in order)"""
    lib.usip_launch_log(1)
    try:
        out, names = call(), []
        while (name := lib.usip_launch_log_entry(len(names), None)) is not None:
            names.append(name.decode())
    finally:
        lib.usip_launch_log(0)
    return out, names


def _bn_layer_inputs(g, nb, C, P, scale=1.0):
    """A pre-BatchNorm tensor with its training-mode forward coefficients [4, C] (scale, shift, mean, invstd)."""
    x = (torch.randn(nb, C, P, generator=g) * scale + 0.3 * torch.randn(1, C, 1, generator=g)).to(DEV)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    mean, var = x.mean((0, 2)), x.var((0, 2), unbiased=False)
    invstd = torch.rsqrt(var + 1e-5)
    coef = torch.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd]).contiguous()
    from usip_amd import ops
    ops.declare_samples(coef, nb * P)                  # what ops.bn_finalize records: the statistics cover these nb * P samples
    return x, gamma, mean.contiguous(), invstd.contiguous(), coef


def _placed_arg(g, nb, C, G, group, edges):
    """arg i32 [nb, C, G]: half of the places random, half drawn from the given edge places."""
    arg = torch.randint(0, group, (nb, C, G), generator=g, dtype=torch.int32)
    edge = torch.tensor(edges, dtype=torch.int32)[torch.randint(0, len(edges), (nb, C, G), generator=g)]
    arg = torch.where(torch.rand(nb, C, G, generator=g) < 0.5, edge, arg)
    for i, k in enumerate(edges):                      # ... and every edge place at least once, whatever the draw
        arg[0, i % C, i % G] = k
    return arg.to(DEV).contiguous()


def _fork_dpooled(g, nb, C, G, big):
    """zeros, negatives, and one value larger than every dense entry (the maximum then comes from the sparse part)"""
    dp = torch.randn(nb, C, G, generator=g)
    dp[torch.rand(nb, C, G, generator=g) < 0.25] = 0.0
    dp[0, 1, 0] = -abs(float(dp[0, 1, 0])) - 0.5
    dp[nb - 1, C - 1, G - 1] = big
    return dp.to(DEV)


# (nb, K, P, fork_group, runs on gemm_x2f).  The dispatcher gives a 256-row operand the 256 x 256 tiles of gemm_x2f.hip only from
# 256 tiles of 128 positions on (usip_mlp_x3p_tile_rows), so nb = 2 with P = 256 / 512 is a launch of the 128-row kernel: there
# the guard must refuse and the old path run.  P = 16384: 128 tiles, one per workgroup.  P = 33792: 264 tiles on 256
# workgroups -- eight of them take a second tile, whose (dp, arg) block was fetched during the first tile's epilogue into the
# other hand-over buffer, with the K-loop pipeline running across the boundary.
GEMM_CASES = [(2, 64, 256, 16, False), (2, 512, 512, 64, False), (2, 64, 16384, 16, True), (2, 512, 16384, 64, True),
              (2, 64, 33792, 16, True), (2, 64, 33792, 64, True), (2, 64, 16384, 32, True)]


@pytest.mark.parametrize("case", GEMM_CASES)
def test_gemm_fork_equals_the_unfused_launch_plus_the_add(case):
    """csrc/gemm_x2f.hip FORK (the h-half of the KNN fusion module's pooled-concat layer: M = 256 rows behind a_offset pooled-first
    weight columns): dX bit-equal to the unfused launch followed by group_max_backward_add_; arg at k = 0 and group - 1, on
    even and on odd positions (the two values of a lane's store), and random; which kernel ran is read from the launch log."""
    from usip_amd import _lib, ops
    nb, K, P, group, takes = case
    M, a_off = 256, 64
    G = P // group
    lib = _lib.lib()
    g = torch.Generator().manual_seed(K + P + group)
    prev = ops.set_matmul_mode("f32x2")
    lib.usip_set_tuning(b"gemm_split3", 2)
    keep_cache, ops.PLANES_CACHE = ops.PLANES_CACHE, {}
    try:
        w2 = (torch.randn(K, a_off + M, generator=g) * (2.0 / K) ** 0.5).to(DEV)      # [Cout][Cp + Ch]: dX = W_h^T . dY
        y, gamma_y, mean_y, invstd_y, coef_y = _bn_layer_inputs(g, nb, K, P)
        dz = torch.randn(nb, K, P, generator=g).to(DEV)
        _, _, coef4, _ = ops.bn_backward_reduce(dz, y, coef_y, mean_y, invstd_y, gamma_y, True)
        assert coef4.shape[0] == 5
        kw = dict(pro=2, X2=y, coef=coef4, tag="dgrad", M=M, a_offset=a_off)
        (dx0, _), ran0 = _launched(lib, lambda: ops.mlp_gemm(w2, dz, **kw))
        assert takes == ("::gemm_x2f_kernel<2, 0, true>(" in ran0[-1]), ran0
        arg = _placed_arg(g, nb, M, G, group, sorted({0, 1, group - 2, group - 1}))
        dp = _fork_dpooled(g, nb, M, G, big=2.0 * float(dx0.abs().max()) + 1.0)
        want = ops.group_max_backward_add_(dx0.clone().view(nb, M, G, group), dp, arg).view(nb, M, P)
        (dx, _, took), ran = _launched(lib, lambda: ops.mlp_gemm(w2, dz, fork=(dp, arg, group), **kw))
        assert took == takes and takes == ("gemm_x2f_fork_kernel" in ran[-1]), ran
        if not takes:
            assert ran[-1] == ran0[-1] and torch.equal(dx, dx0)          # the old path: the caller still has the add to do
            return
        assert lib.usip_mlp_gemm_x2h_fork_supported(M, K, P, nb, group) == 1
        assert torch.equal(dx, want), float((dx - want).abs().max())
        dx2 = ops.mlp_gemm(w2, dz, fork=(dp, arg, group), **kw)[0]
        assert torch.equal(dx2, dx)
        # the switch restores the unfused launch
        keep = ops.POOL_GRAD_FOLD
        ops.POOL_GRAD_FOLD = False
        try:
            (dx3, _, took3), ran3 = _launched(lib, lambda: ops.mlp_gemm(w2, dz, fork=(dp, arg, group), **kw))
        finally:
            ops.POOL_GRAD_FOLD = keep
        assert not took3 and ran3[-1] == ran0[-1] and torch.equal(dx3, dx0)
    finally:
        ops.PLANES_CACHE = keep_cache
        lib.usip_set_tuning(b"gemm_split3", 0)
        ops.set_matmul_mode(prev)


def test_gemm_fork_guards_keep_the_old_path():
    """f32 mode, a run length the kernel does not take (8, 128), and rows that are no multiple of 256: the unfused launch runs
    (launch log), the call says it did nothing about the fork, and dX is the unfused dX."""
    from usip_amd import _lib, ops
    lib = _lib.lib()
    nb, K, P = 2, 64, 16384
    g = torch.Generator().manual_seed(11)
    y, gamma_y, mean_y, invstd_y, coef_y = _bn_layer_inputs(g, nb, K, P)
    dz = torch.randn(nb, K, P, generator=g).to(DEV)
    _, _, coef4, _ = ops.bn_backward_reduce(dz, y, coef_y, mean_y, invstd_y, gamma_y, True)
    keep_cache, ops.PLANES_CACHE = ops.PLANES_CACHE, {}
    try:
        for mode, M, group in (("f32", 256, 16), ("f32x2", 256, 8), ("f32x2", 256, 128), ("f32x2", 192, 16), ("f32x3", 256, 16)):
            prev = ops.set_matmul_mode(mode)
            lib.usip_set_tuning(b"gemm_split3", 2 if mode != "f32" else 0)
            try:
                w2 = (torch.randn(K, M, generator=g) * 0.2).to(DEV)
                G = P // group
                arg = torch.randint(0, group, (nb, M, G), generator=g, dtype=torch.int32).to(DEV)
                dp = torch.randn(nb, M, G, generator=g).to(DEV)
                kw = dict(pro=2, X2=y, coef=coef4, tag="dgrad")
                (dx0, _), ran0 = _launched(lib, lambda: ops.mlp_gemm(w2, dz, **kw))
                (dx, _, took), ran = _launched(lib, lambda: ops.mlp_gemm(w2, dz, fork=(dp, arg, group), **kw))
                assert not took and ran[-1] == ran0[-1] and "fork" not in ran[-1], (mode, M, group, ran)
                assert torch.equal(dx, dx0)
                assert lib.usip_mlp_gemm_x2h_fork_supported(M, K, P, nb, group) == 0 or mode != "f32x2"
            finally:
                lib.usip_set_tuning(b"gemm_split3", 0)
                ops.set_matmul_mode(prev)
    finally:
        ops.PLANES_CACHE = keep_cache


def _micro_step(fold, mode, graph=False, calls=3):
    """The detector_ball_micro step with the fold on / off -> (DetectorStep, number of stand-alone pooling-gradient passes)"""
    from usip_amd import _lib, ops, synth
    from usip_amd.networks import DetectorOptions
    from usip_amd.step import DetectorStep, batch_to_device
    g = load_golden("detector_ball_micro.npz")
    opt = DetectorOptions(surface_normal_len=g["in/src_sn"].shape[1], node_knn_k_1=int(g["cfg_knn"]),
                          loss_sigma_lower_bound=float(g["cfg_sigma_lb"]), keypoint_on_pc_alpha=float(g["cfg_alpha"]))
    prev = ops.set_matmul_mode(mode)
    if mode != "f32":
        _lib.lib().usip_set_tuning(b"gemm_split3", 2)
    keep, ops.POOL_GRAD_FOLD = ops.POOL_GRAD_FOLD, fold
    count = [0]
    real = ops.group_max_backward_add_

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    ops.group_max_backward_add_ = counted
    try:
        st = DetectorStep(str(g["cfg_model"]), opt, DEV, graph=graph)
        sd = st.detector.state_dict()
        st.load_numpy_state(synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()}))
        batch = batch_to_device({k[3:]: v for k, v in g.items() if k.startswith("in/")}, DEV)
        for _ in range(calls if graph else 1):             # graph: calls 1-2 eager, call 3 captures and replays
            st.step(batch)
        torch.cuda.synchronize()
        return st, count[0]
    finally:
        ops.group_max_backward_add_ = real
        ops.POOL_GRAD_FOLD = keep
        _lib.lib().usip_set_tuning(b"gemm_split3", 0)
        ops.set_matmul_mode(prev)


def _assert_same_step(on, off):
    for k in ("loss", "keypoints", "sigmas", "node"):
        assert torch.equal(on.last[k], off.last[k]), k
    for k, v in on.detector.last_indices.items():
        assert torch.equal(v, off.detector.last_indices[k]), k
    goff = dict(off.detector.named_parameters())
    for k, p in on.detector.named_parameters():
        assert torch.equal(p.grad, goff[k].grad), k
    assert torch.equal(on.bucket.flat, off.bucket.flat)
    sd = off.detector.state_dict()
    for k, v in on.detector.state_dict().items():          # forward untouched: BatchNorm buffers too
        assert torch.equal(v, sd[k]), k


def test_whole_step_with_the_fold_equals_the_step_without_it():
    """detector_ball_micro in f32x2, fold on against ops.POOL_GRAD_FOLD = False: every forward output, index tensor and
    parameter gradient bit-equal (conv1-conv3 included: the front end keeps its stand-alone pass).  At this size the KNN
    fusion's launch is one the guard refuses (the 128-row kernel), so both stand-alone passes run either way; the step below
    is the smallest whose launch takes the fold."""
    on, n_on = _micro_step(True, "f32x2")
    off, n_off = _micro_step(False, "f32x2")
    print("stand-alone pooling-gradient passes per step: fold off", n_off, "fold on", n_on)
    assert n_off == 2 and n_on == 2
    _assert_same_step(on, off)


def _fold_sized_step(fold, graph=False):
    """2 pairs of 4096 points with 512 nodes, K = 16: the KNN fusion's data gradient is 256 rows x (4 clouds x 8192 positions)
    = 256 tiles of 128, the first size gemm_x2f.hip takes -> (DetectorStep, number of stand-alone passes)"""
    from usip_amd import _lib, ops, synth
    from usip_amd.networks import DetectorOptions
    from usip_amd.step import DetectorStep, batch_to_device
    lib = _lib.lib()
    opt = DetectorOptions(surface_normal_len=4, node_knn_k_1=16)
    prev = ops.set_matmul_mode("f32x2")
    lib.usip_set_tuning(b"gemm_split3", 2)
    keep, ops.POOL_GRAD_FOLD = ops.POOL_GRAD_FOLD, fold
    count = [0]
    real = ops.group_max_backward_add_

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    ops.group_max_backward_add_ = counted
    try:
        st = DetectorStep("ball", opt, DEV, graph=graph)
        sd = st.detector.state_dict()
        st.load_numpy_state(synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()}))
        batch = batch_to_device(synth.make_pair_batch(7, 2, 4096, 512, 4, "slab"), DEV)
        for _ in range(3 if graph else 1):                 # graph: calls 1-2 eager, call 3 captures and replays
            st.step(batch)
        torch.cuda.synchronize()
        return st, count[0]
    finally:
        ops.group_max_backward_add_ = real
        ops.POOL_GRAD_FOLD = keep
        lib.usip_set_tuning(b"gemm_split3", 0)
        ops.set_matmul_mode(prev)


def test_step_whose_launch_takes_the_fold_equals_the_step_without_it():
    """The Ball step at the smallest size whose KNN-fusion data gradient runs on gemm_x2f.hip, in f32x2: with the fold on one
    stand-alone pass is gone (the guard said yes and mlp_gemm reported the fold taken, or the pass would have run), and the
    whole step -- outputs, indices, every parameter gradient, BatchNorm buffers -- is bit-equal to the step without it;
    replayed from its captured graph it is the eager step."""
    from usip_amd import _lib
    assert _lib.lib().usip_mlp_gemm_x2h_fork_supported(256, 512, 512 * 16, 4, 16) == 1
    on, n_on = _fold_sized_step(True)
    off, n_off = _fold_sized_step(False)
    assert n_off == 2 and n_on == 1, (n_off, n_on)
    _assert_same_step(on, off)
    graph, _ = _fold_sized_step(True, graph=True)
    assert len(graph._graphs) == 1
    for k in ("loss", "keypoints", "sigmas"):
        assert torch.equal(graph.last[k], on.last[k]), k
    assert torch.equal(graph.bucket.flat, on.bucket.flat)


def test_whole_step_graph_replay_equals_eager_with_the_fold():
    """Fold on: the step replayed from its captured HIP graph is the eager step, bit for bit (loss, keypoints, every gradient)."""
    eager, _ = _micro_step(True, "f32x2")
    graph, _ = _micro_step(True, "f32x2", graph=True)
    assert len(graph._graphs) == 1
    for k in ("loss", "keypoints", "sigmas"):
        assert torch.equal(graph.last[k], eager.last[k]), k
    assert torch.equal(graph.bucket.flat, eager.bucket.flat)


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_whole_step_in_the_other_modes_keeps_the_old_path(mode):
    """f32 / f32x3: no launch can take the fold, both stand-alone passes run, and the switch changes nothing at all."""
    on, n_on = _micro_step(True, mode)
    off, n_off = _micro_step(False, mode)
    assert n_on == 2 and n_off == 2
    assert torch.equal(on.last["loss"], off.last["loss"])
    assert torch.equal(on.bucket.flat, off.bucket.flat)
