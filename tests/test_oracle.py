"""CPU tests: the oracle (oracle/) against the golden vectors made from the reference.

The oracle is test infrastructure; these tests are what entitles the GPU parity tests to use
it as the checker.  index_max is pinned by the reference's own C++ (built unmodified);
torch-level functions are pinned by fixtures captured from the reference's Python modules;
ball_query is a line-by-line restatement with NO executable reference ("parity unpinned").
"""
import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden
from oracle import detector as od
from oracle import native

IM_TAGS = ["random", "ties", "floor", "empty", "nan", "tiny", "n_lt_wave"]


@pytest.mark.parametrize("tag", IM_TAGS)
def test_index_max_oracle_matches_reference_cpp(tag):
    g = load_golden("index_max_cases.npz")
    out = native.index_max(g[tag + "_data"], g[tag + "_index"], int(g[tag + "_K"]))
    assert np.array_equal(out, g[tag + "_out"])


def test_index_max_oracle_matches_live_reference_build():
    """Two random cases (seed 7) against the reference's own C++: its recorded outputs
    (index_max_live_cases.npz), and, when oracle/_ref/index_max.so is present, a live call too."""
    from oracle.build_ref import load_ref_index_max
    g = load_golden("index_max_live_cases.npz")
    ref = load_ref_index_max()
    for tag in ("small", "wide"):
        d, i, K = g[tag + "_data"], g[tag + "_index"], int(g[tag + "_K"])
        assert np.array_equal(native.index_max(d, i, K), g[tag + "_out"]), tag
        if ref is not None:
            want = ref.forward_cpu(torch.from_numpy(d), torch.from_numpy(i), K).numpy()
            assert np.array_equal(want, g[tag + "_out"]), tag


def test_pairwise_dist_oracle_is_bit_exact_vs_torch_norm():
    g = load_golden("dist_ball_cases.npz")
    d = native.pairwise_dist(g["node"], g["x"])
    assert np.array_equal(d, g["dist"])


def test_ball_query_oracle_reproduces_fixture_and_semantics():
    g = load_golden("dist_ball_cases.npz")
    K, r = int(g["K"]), float(g["radius"])
    out, prefix = native.ball_query(g["dist"], r, K, return_prefix=True)
    assert np.array_equal(out, g["ball_idx_unpinned"])
    assert np.array_equal(prefix, g["prefix_len_unpinned"])
    # independent numpy statement of ball_query_cuda.cu:22-46
    dist = g["dist"]
    for b in range(dist.shape[0]):
        for m in range(dist.shape[1]):
            hits = np.nonzero(dist[b, m] <= np.float32(r))[0][:K]
            if len(hits) == 0:
                want = np.zeros(K, np.int32)
            else:
                want = hits[np.arange(K) % len(hits)] if len(hits) < K else hits
            assert np.array_equal(out[b, m], want), (b, m)


def test_som_assign_matches_reference_query_topk():
    g = load_golden("som_cases.npz")
    min_idx, count = od.som_assign(torch.from_numpy(g["node"]), torch.from_numpy(g["x"]))
    assert np.array_equal(min_idx.numpy(), g["min_idx"])
    assert np.array_equal(count.numpy(), g["count"])
    assert np.array_equal((count > 0).numpy().astype(np.int32), g["mask_row_max"])


def test_losses_oracle_matches_reference():
    g = load_golden("losses_cases.npz")
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    src, dst = t["pc_src"].requires_grad_(True), t["pc_dst"].requires_grad_(True)
    ss, sd = t["pc_ss"].requires_grad_(True), t["pc_sd"].requires_grad_(True)
    loss, pure, weighted, _, _ = od.chamfer_prob(src, dst, ss, sd)
    loss.backward()
    assert_close(loss.detach(), g["pc_loss"], name="loss")
    assert_close(pure, g["pc_pure"], name="pure")
    assert_close(weighted, g["pc_weighted"], name="weighted")
    for got, key in ((src.grad, "pc_gsrc"), (dst.grad, "pc_gdst"), (ss.grad, "pc_gss"), (sd.grad, "pc_gsd")):
        assert_close(got, g[key], name=key)
    kp = t["ss_kp"].requires_grad_(True)
    d = od.chamfer_single_side(kp, t["ss_pc"])
    d.backward(t["ss_gd"])
    assert_close(d.detach(), g["ss_d"], name="ss_d")
    assert_close(kp.grad, g["ss_gkp"], name="ss_gkp")


def test_point_to_plane_oracle_matches_reference():
    """PointOnSurfaceLoss (losses.py:146-187) -- selected by opt.keypoint_on_pc_type == 'point_to_plane'
    (keypoint_detector.py:197-201): the oracle's restatement against values and gradient captured from the reference."""
    g = load_golden("point_to_plane_cases.npz")
    kp = torch.from_numpy(g["kp"]).requires_grad_(True)
    loss = od.point_on_surface(kp, torch.from_numpy(g["pc"]), torch.from_numpy(g["sn"]))
    assert tuple(loss.shape) == tuple(g["loss"].shape)
    loss.backward(torch.from_numpy(g["g"]))
    assert_close(loss.detach(), g["loss"], name="point-to-plane loss")
    assert_close(kp.grad, g["gkp"], name="point-to-plane d/dkp")


def _params_from_fixture(g):
    shapes = {k[len("grad_norm/"):]: None for k in g if k.startswith("grad_norm/")}
    return shapes


def _run_step(fix):
    from usip_amd import synth
    from usip_amd.networks import detector_param_shapes
    g = load_golden(fix)
    model = str(g["cfg_model"])
    cs = g["in/src_sn"].shape[1]
    shapes = detector_param_shapes(model, cs)
    filled = synth.fill_parameters(shapes)
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in filled.items()
         if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))}
    bufs = {k: torch.from_numpy(v.copy()) for k, v in filled.items()
            if k.endswith("running_mean") or k.endswith("running_var")}
    batch = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("in/")}
    res = od.detector_step(P, bufs, batch, model, int(g["cfg_knn"]), float(g["cfg_sigma_lb"]),
                           float(g["cfg_alpha"]))
    return g, P, bufs, res


@pytest.mark.parametrize("fix", ["detector_som_cfg1.npz", "detector_ball_micro.npz", "detector_som_micro.npz",
                                 "detector_lite_micro.npz", "detector_knn_micro.npz"])
def test_detector_step_oracle_matches_reference(fix):
    g, P, bufs, res = _run_step(fix)
    # indices: bit-exact
    if "idx/min_idx" in g:
        assert np.array_equal(res["min_idx"].numpy(), g["idx/min_idx"])
        assert np.array_equal(res["first_idx"].numpy(), g["idx/index_max_0"])
        assert np.array_equal(res["second_idx"].numpy(), g["idx/index_max_1"])
    if "idx/ball_idx" in g:
        assert np.array_equal(res["ball_idx"].numpy(), g["idx/ball_idx"])
    if "idx/nn_idx" in g:      # RPN_Detector_KNN: the SET of the reference's topk(sorted=False), in canonical order
        assert np.array_equal(res["nn_idx"].numpy(), g["idx/nn_idx"])
    assert np.array_equal(res["knn_I"].numpy(), g["idx/knn_I"])
    # the arg-max of every max-pool over K (the position the gradient is routed to), as the reference's own
    # torch.max returned it
    n_pools = sum(k.startswith("idx/pool_arg_") for k in g)
    assert n_pools == len(res["pool_args"]) == (4 if ("idx/ball_idx" in g or "idx/nn_idx" in g) else 2)
    for i, arg in enumerate(res["pool_args"]):
        same = arg.numpy() == g["idx/pool_arg_%d" % i].astype(np.int64)
        if "idx/nn_idx" in g and i < 2:
            # RPN_Detector_KNN: torch.max returns the FIRST maximum, and "first" is a position in the reference's own
            # (unspecified) neighbour order -- where several neighbours tie (channels that are zero after the ReLU
            # for a whole neighbourhood) the fixture's choice, re-expressed in the canonical order, is another of
            # the maxima.  Checked below: routing through the fixture's choices reproduces the forward bit for bit.
            assert same.mean() > 0.97, (i, same.mean())
        else:
            assert same.all(), i
    if "idx/nn_idx" in g:
        od.TAPE = od.DecisionTape(pools=[torch.from_numpy(g["idx/pool_arg_%d" % i].astype(np.int64)) for i in range(n_pools)])
        try:
            _, _, _, pinned = _run_step(fix)
        finally:
            od.TAPE = None
        for k in ("keypoints", "sigmas", "loss"):
            assert torch.equal(pinned[k], res[k]), k
    # floats: 1e-5 relative
    for k in ("node", "keypoints", "sigmas", "loss", "loss_chamfer", "chamfer_pure", "chamfer_weighted",
              "loss_on_pc_src", "loss_on_pc_dst"):
        assert_close(res[k].detach().numpy(), g[k], name=k)
    biggest = max(float(v) for k, v in g.items() if k.startswith("grad_norm/"))
    for k, p in P.items():
        gr = p.grad.numpy().ravel().astype(np.float64)
        gn = float(g["grad_norm/" + k])
        if gn < 1e-5 * biggest:
            # analytically zero gradient (a conv bias whose effect a later BatchNorm removes): what
            # autograd returns is rounding noise, not a value to match
            continue
        assert_close(np.sqrt((gr ** 2).sum()), gn, rel=2e-5, name="grad_norm/" + k)
        scale = max(np.abs(gr).max(), 1e-30)
        err = np.abs(gr[:48] - g["grad_head/" + k].astype(np.float64)).max() / scale
        assert err <= 2e-5, (k, err)
        # four +-1 projections of the WHOLE gradient (normalised by sqrt(len): an entry-wise error e shows up as ~e)
        from usip_amd import synth
        proj = synth.grad_projections(k, gr)
        assert np.abs(proj - g["grad_proj/" + k]).max() <= 2e-5 * scale, (k, proj, g["grad_proj/" + k])
    for k, v in bufs.items():
        assert_close(v.numpy(), g["buf/" + k], name=k)


def _descriptor_inputs(g):
    from usip_amd import synth
    from usip_amd.networks import DescriptorLiteOld, DetectorOptions
    opt = DetectorOptions(surface_normal_len=4)
    shapes = {k: tuple(v.shape) for k, v in DescriptorLiteOld(opt).state_dict().items()}
    filled = synth.fill_parameters(shapes)
    batch = {k: torch.from_numpy(g[k]) for k in ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "anc_kp", "pos_kp",
                                                 "anc_sigmas", "neg_idx")}
    return opt, filled, batch


def test_descriptor_step_oracle_matches_reference():
    """oracle restatement of DescriptorLiteOld + DescPairScanLoss against the fixture captured
    from the reference (ball indices from the unpinned ball_query restatement)."""
    g = load_golden("descriptor_micro.npz")
    opt, filled, batch = _descriptor_inputs(g)
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in filled.items()
         if not ("running_" in k or "num_batches" in k)}
    bufs = {k: torch.from_numpy(v.copy()) for k, v in filled.items() if "running_" in k}
    res = od.descriptor_step(P, bufs, batch, torch.from_numpy(g["perm"]))
    for k in ("descriptors", "x_features", "triplet", "active", "loss"):
        assert_close(res[k].detach().numpy(), g[k], rel=1e-6, name=k)
    for k, p in P.items():
        gn = float(g["grad_norm/" + k])
        if gn < 1e-5 * max(float(v) for kk, v in g.items() if kk.startswith("grad_norm/")):
            continue
        assert_close(p.grad.numpy().ravel()[:48], g["grad_head/" + k], rel=1e-5, name=k)


def test_fps_and_nms_oracles_match_reference_functions():
    """f-3 / f-4: numpy restatements against outputs of the reference's own FarthestSampler and nms()."""
    from oracle import postproc
    g = load_golden("pre_post_cases.npz")
    for b in range(g["fps_pts"].shape[0]):
        idx = postproc.fps_indices(g["fps_pts"][b], int(g["fps_first"][b]), g["fps_idx"].shape[1])
        assert np.array_equal(idx, g["fps_idx"][b])
    for b in range(2):
        order = postproc.nms_order(g["nms_kp"][b], g["nms_sigma"][b], float(g["nms_radius"]))
        assert np.array_equal(g["nms_kp"][b][order], g["nms_kept_%d" % b])
        assert np.array_equal(g["nms_sigma"][b][order], g["nms_sigma_%d" % b])
        top = postproc.export_keypoints(g["nms_kp"][b], g["nms_sigma"][b], float(g["nms_radius"]), 40)
        assert np.array_equal(top, g["nms_top40_%d" % b])


def test_checkpoint_prefix_fixup_and_bin_format(tmp_path):
    """f-4 host logic: 'module.'-prefixed checkpoints load (kitti/train_detector.py:42-51); the .bin file is
    float32 M x 3 row-major (save_keypoints.py:392-393)."""
    from usip_amd import inference
    from usip_amd.networks import DetectorOptions, build_detector
    net = build_detector("som", DetectorOptions(surface_normal_len=3))
    sd = {"module." + k: v.clone() + 1 for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    sd.update({"module." + k: v for k, v in net.state_dict().items() if not v.dtype.is_floating_point})
    inference.load_detector_state(net, sd)
    assert torch.equal(net.mlp3.conv.bias, sd["module.mlp3.conv.bias"])
    kp = np.arange(12, dtype=np.float64).reshape(4, 3)
    path = str(tmp_path / "000001.bin")
    inference.write_keypoints_bin(path, kp)
    back = np.fromfile(path, dtype=np.float32).reshape(-1, 3)
    assert np.array_equal(back, kp.astype(np.float32))


def test_ball_query_oracle_matches_reference_numba_ancestor():
    """Pins the ball_query oracle to the reference's own statement of the algorithm: the numba-CUDA kernel it
    keeps (commented out) at models/operations.py:295-329, executed by tests/golden/make_golden.py through a
    thread-index shim.  The ancestor is undefined for an empty ball (modulo by the hit count); those rows follow
    the CUDA kernel's rule, all zeros (ball_query_cuda.cu:40-45)."""
    g = load_golden("ball_query_ancestor_cases.npz")
    for n in "abc":
        dist, K, r = g[n + "_dist"], int(g[n + "_K"]), float(g[n + "_radius"])
        out = native.ball_query(dist, r, K)
        empty = g[n + "_empty"]
        assert np.array_equal(out[~empty], g[n + "_idx"][~empty]), n
        assert not out[empty].any()
        assert empty.any() and (~empty).any()

