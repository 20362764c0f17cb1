"""The indoor descriptor head's host-side surface (usip_amd.networks.DescriptorLiteOldGlobal, IndoorOptions,
usip_amd.step.IndoorDescriptorStep) and the fixture tests/golden/indoor_head.npz, without a GPU.  The numbers are held to the
fixture in tests/test_indoor_head_gpu.py."""
import numpy as np
import pytest
import torch

import indoor_oracle as io_
from conftest import load_golden


def _options(g, **kw):
    from usip_amd.networks import IndoorOptions
    return IndoorOptions(descriptor_len=float(g["cfg_descriptor_len"]), ball_radius=float(g["cfg_ball_radius"]),
                         ball_nsamples=int(g["cfg_ball_nsamples"]), CGF_radius=float(g["cfg_CGF_radius"]),
                         triple_loss_gamma=float(g["cfg_triple_loss_gamma"]), sigma_max=float(g["cfg_sigma_max"]), **kw)


def test_state_dict_has_the_references_keys_and_shapes():
    from usip_amd.networks import DescriptorLiteOldGlobal
    g = load_golden("indoor_head.npz")
    net = DescriptorLiteOldGlobal(_options(g))                           # descriptor_len arrives as a float, as the indoor options declare it
    sd = net.state_dict()
    assert len(sd) == 46
    params = {k: tuple(p.shape) for k, p in net.named_parameters()}
    assert params == {k[len("grad/"):]: tuple(v.shape) for k, v in g.items() if k.startswith("grad/")}
    buffers = {k: tuple(v.shape) for k, v in sd.items() if k.endswith("running_mean") or k.endswith("running_var")}
    assert buffers == {k[len("buf/"):]: tuple(v.shape) for k, v in g.items() if k.startswith("buf/")}
    layers = sorted({k.split(".")[0] for k in sd})
    assert layers == ["conv1", "conv2", "conv3", "conv4", "conv5", "fc1", "fc2", "fc3"]
    assert all(k.split(".")[1] in ("conv", "norm") for k in sd)
    assert not any(k.startswith(("conv5.norm", "fc3.norm")) for k in sd)


def test_a_reference_layout_checkpoint_loads_strictly():
    from usip_amd import inference
    from usip_amd.networks import DescriptorLiteOldGlobal
    g = load_golden("indoor_head.npz")
    rng = np.random.default_rng(0)
    ckpt = {}
    for k, v in g.items():
        if k.startswith("grad/"):
            ckpt[k[len("grad/"):]] = torch.from_numpy(rng.standard_normal(v.shape).astype(np.float32))
        elif k.startswith("buf/"):
            ckpt[k[len("buf/"):]] = torch.from_numpy(v.copy())
            if k.endswith("running_mean"):
                ckpt[k[len("buf/"):-len("running_mean")] + "num_batches_tracked"] = torch.tensor(1, dtype=torch.int64)
    assert len(ckpt) == 46
    net = DescriptorLiteOldGlobal(_options(g))
    res = net.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.fc1.conv.weight.data, ckpt["fc1.conv.weight"])
    assert torch.equal(net.fc2.norm.running_var, ckpt["fc2.norm.running_var"])
    # ... and as nn.DataParallel saved it
    net2 = DescriptorLiteOldGlobal(_options(g))
    inference.load_detector_state(net2, {"module." + k: v for k, v in ckpt.items()})
    assert torch.equal(net2.conv4.conv.weight.data, ckpt["conv4.conv.weight"])


def test_the_fixture_satisfies_its_generators_conditions():
    g = load_golden("indoor_head.npz")
    figures = io_.fixture_conditions(g)
    print(figures)
    assert (int(g["cfg_ball_nsamples"]), int(g["cfg_descriptor_len"]), g["anc_kp"].shape) == (448, 64, (2, 3, 24))
    assert sum(k.startswith("idx/pool_arg_") for k in g) == 3 and sum(k.startswith("idx/relu_near_idx_") for k in g) == 6
    assert g["idx/pool_arg_2"].shape == (4, 64)                          # the pool over the keypoints
    # the keypoints' transform as the step applies it: R . kp * s + t
    moved = np.einsum("bij,bjm->bim", g["anc_R_pos"].astype(np.float64), g["anc_kp"].astype(np.float64)) \
        * g["anc_scale_pos"].astype(np.float64)[:, :, None] + g["anc_shift_pos"]
    assert np.abs(moved - g["anc_kp_moved"]).max() < 1e-6
    d = np.linalg.norm(g["descriptors"].astype(np.float64), axis=1)
    assert np.abs(d - 1).max() < 1e-4 and np.abs(np.linalg.norm(g["descriptors_eval"].astype(np.float64), axis=1) - 1).max() < 1e-4
    assert np.isclose(float(g["loss"]), float(g["triplet"].mean()), rtol=1e-6)


def test_indoor_options_are_the_references():
    from usip_amd.networks import IndoorOptions
    o = IndoorOptions()
    assert (o.input_pc_num, o.node_num, o.ball_radius, o.ball_nsamples) == (5000, 512, 0.75, 448)
    assert (o.descriptor_len, o.CGF_radius, o.triple_loss_gamma, o.sigma_max) == (128, 0.075, 0.3, 0.5)
    assert (o.surface_normal_len, o.lr, o.batch_size, o.random_pc_dropout_lower_limit) == (4, 0.001, 2, 1.0)
    assert IndoorOptions(lr=0.01).lr == 0.01


def test_host_tensors_and_the_dropout_option_are_refused():
    from usip_amd.networks import DescriptorLiteOldGlobal, IndoorOptions
    from usip_amd.step import IndoorDescriptorStep
    net = DescriptorLiteOldGlobal(IndoorOptions(descriptor_len=16, ball_nsamples=8))
    with pytest.raises(RuntimeError, match="device tensors"):
        net(torch.zeros(1, 3, 32), torch.zeros(1, 4, 32), torch.zeros(1, 3, 4))
    with pytest.raises(NotImplementedError, match="random_pc_dropout_lower_limit"):
        IndoorDescriptorStep(IndoorOptions(random_pc_dropout_lower_limit=0.5), "cpu")


def test_head_tail_restatement_matches_torch_modules():
    """tests/indoor_oracle.py::head_tail against nn.Conv1d / nn.BatchNorm1d / ReLU strung together: the GPU tests' float64
    reference is the head the reference writes."""
    from usip_amd.networks import DescriptorLiteOldGlobal, IndoorOptions
    torch.manual_seed(1)
    net = DescriptorLiteOldGlobal(IndoorOptions(descriptor_len=8, ball_nsamples=8)).double()
    d = torch.randn(3, 8, 5, dtype=torch.float64)
    P = {k: v for k, v in net.state_dict().items() if k.startswith("fc")}
    got = io_.head_tail(d, P, training=True)
    h = torch.cat((d, d.max(dim=2, keepdim=True)[0].expand(3, 8, 5)), 1)
    for fc in (net.fc1, net.fc2):
        h = torch.relu(torch.nn.functional.batch_norm(fc.conv(h), None, None, fc.norm.weight, fc.norm.bias, True, 0.0, 1e-5))
    h = net.fc3.conv(h)
    want = h / (torch.norm(h, dim=1, keepdim=True) + 1e-5)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
