"""GPU tests of describing fragments from checkpoints (usip_amd.fragment_batch.FragmentDescriber): against the
existing calls it strings together, the padding by the first pick, a fragment in a batch against the fragment alone, a
synthetic scene end to end through FragmentEvaluator, the files, and that nothing synchronises with the host."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_fragment_batch_cpu import fixture_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, M, TOP, SAMPLES, D = 1024, 64, 32, 64, 64
# Chosen on the device so that the margins test_a_fragment_in_a_batch_equals_the_fragment_alone asserts hold: the builder's
# seed decides the points and so the keypoints; NMS_RADIUS is in the units of the 6 m slab the fixture's frames are cut from.
BUILDER_SEED, NMS_RADIUS = 4, 0.6
MARGIN = 1e-4


@pytest.fixture(scope="module")
def g():
    return load_golden("fragment_batch_cases.npz")


def networks():
    """A seeded Ball detector (synth.fill_parameters) and a seeded DescriptorLiteOldGlobal; neither is trained."""
    from usip_amd import synth
    from usip_amd.networks import DescriptorLiteOldGlobal, IndoorOptions, build_detector
    opt = IndoorOptions(input_pc_num=N, node_num=M, descriptor_len=D, node_knn_k_1=16, ball_nsamples=SAMPLES)
    det = build_detector("ball", opt)
    sd = det.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    det.load_state_dict({k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in filled.items()})
    torch.manual_seed(5)
    return det.to(DEV).eval(), DescriptorLiteOldGlobal(opt).to(DEV).eval(), opt


@pytest.fixture(scope="module")
def world(g):
    from usip_amd import fragment_batch as fb
    det, desc, opt = networks()
    bank = fb.FragmentScanBank.from_arrays(fixture_frames(g), DEV)
    recipe = fb.FragmentBatchRecipe.match3d(opt)
    assert (recipe.N, recipe.n_sub, recipe.M, recipe.Cs) == (N, N // 2, M, 4)
    builder = fb.FragmentBatchBuilder(bank, recipe, seed=BUILDER_SEED)
    describer = fb.FragmentDescriber(det, desc, builder, nms_radius=NMS_RADIUS, top=TOP)
    return dict(det=det, desc=desc, bank=bank, builder=builder, describer=describer)


def test_describer_equals_the_existing_calls_bit_for_bit(world):
    from usip_amd import inference
    from usip_amd.evaluation import select_keypoints_device
    ids = [0, 2, 3]
    batch = world["builder"].build(ids, 0)
    keypoints, sigmas = inference.run_model(world["det"], batch["pc"], batch["sn"], batch["node"])
    kp, count = select_keypoints_device(keypoints, sigmas, NMS_RADIUS, TOP)
    desc = inference.describe_keypoints(world["desc"], batch["pc"], batch["sn"], kp, perm_seed=0)
    out = world["describer"].describe(ids)
    for k in ("pc", "sn", "node"):
        assert torch.equal(out[k], batch[k]), k
    assert torch.equal(out["keypoints"], keypoints) and torch.equal(out["sigmas"], sigmas)
    assert torch.equal(out["kp"], kp) and torch.equal(out["count"], count) and torch.equal(out["desc"], desc)
    assert out["kp"].shape == (3, 3, TOP) and out["desc"].shape == (3, D, TOP) and out["count"].dtype == torch.int32
    only = world["describer"].keypoints(ids)
    assert "desc" not in only and torch.equal(only["kp"], kp) and torch.equal(only["count"], count)
    again = world["describer"].describe_keypoints(ids, kp, count)
    assert torch.equal(again["desc"], desc) and torch.equal(again["count"], count)
    assert torch.allclose(desc.norm(dim=1), torch.ones_like(desc[:, 0]), atol=1e-4)


def test_padding_by_the_first_pick_does_not_alter_the_global_max(world):
    """A radius wide enough that NMS leaves fewer than `top` keypoints: the padded columns repeat the first pick, whose
    descriptor is already under the max over the keypoints, so the first `count` columns are those of describing exactly
    the `count` keypoints."""
    from usip_amd import fragment_batch as fb, inference
    wide = fb.FragmentDescriber(world["det"], world["desc"], world["builder"], nms_radius=2.5, top=TOP)
    out = wide.describe([1])
    n = int(out["count"][0])
    print("count %d of top %d" % (n, TOP))
    assert 1 <= n < TOP
    assert torch.equal(out["kp"][0, :, n:], out["kp"][0, :, :1].expand(3, TOP - n))
    alone = inference.describe_keypoints(world["desc"], out["pc"], out["sn"], out["kp"][:, :, :n].contiguous(), perm_seed=0)
    err = float((out["desc"][0, :, :n] - alone[0]).abs().max())
    print("largest difference %.3e" % err)
    assert err <= 1e-5


def margins(keypoints, sigmas, radius):
    """(smallest relative gap between two neighbouring sigmas, smallest |distance - radius| / radius over every pair of
    keypoints) of one fragment: every comparison the sigma-ordered NMS can make, the ones it does make among them."""
    s = np.sort(sigmas.astype(np.float64))
    gap = float(((s[1:] - s[:-1]) / s[1:]).min())
    p = keypoints.astype(np.float64).T
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))[np.triu_indices(p.shape[0], 1)]
    return gap, float((np.abs(d - radius) / radius).min())


def test_a_fragment_in_a_batch_equals_the_fragment_alone(world):
    three = world["describer"].describe([1, 2, 0])
    one = world["describer"].describe([2])
    torch.cuda.synchronize()
    gap, edge = margins(one["keypoints"][0].cpu().numpy(), one["sigmas"][0].cpu().numpy(), NMS_RADIUS)
    print("sigma gap %.3e, NMS edge %.3e" % (gap, edge))
    assert gap > MARGIN and edge > MARGIN
    assert torch.equal(three["pc"][1], one["pc"][0]) and torch.equal(three["node"][1], one["node"][0])
    assert int(three["count"][1]) == int(one["count"][0])
    n = int(one["count"][0])
    scale = float(one["kp"][0].abs().max())
    kp_err = float((three["kp"][1] - one["kp"][0]).abs().max()) / scale
    order3 = torch.argsort(three["sigmas"][1], stable=True)
    order1 = torch.argsort(one["sigmas"][0], stable=True)
    assert torch.equal(order3, order1)
    desc_err = float((three["desc"][1, :, :n] - one["desc"][0, :, :n]).abs().max())
    print("kp %.3e desc %.3e" % (kp_err, desc_err))
    assert kp_err <= 1e-5 and desc_err <= 1e-5


@pytest.fixture(scope="module")
def scene():
    """4 fragments x 4000 xyz rows of the synthetic room, with its ground truth."""
    from usip_amd import fragments as fr
    return fr.synthetic_scene(seed=2, fragments=4, points=4000, dim=D)


def test_a_synthetic_scene_end_to_end_and_the_files(world, scene, tmp_path):
    from usip_amd import fragment_batch as fb, fragments as fr, inference
    clouds = [np.asarray(c, np.float32)[:, :3] for c in scene["clouds"]]
    assert len(clouds) == 4
    bank = fb.FragmentScanBank.from_arrays(clouds, DEV)
    assert bank.row_len == 7
    builder = fb.FragmentBatchBuilder(bank, world["builder"].recipe, seed=1)
    describer = fb.FragmentDescriber(world["det"], world["desc"], builder, nms_radius=0.3, top=TOP)
    kw = dict(top=TOP, max_trials=2000, seed=0, batch_pairs=8)
    a = fr.FragmentEvaluator(None, None, None, DEV, **kw)
    b = fr.FragmentEvaluator(None, None, None, DEV, **kw)
    for ids in ([0, 1, 2], [3]):
        out = describer.describe(ids)
        a.add_described(ids, out["kp"], out["desc"], out["count"], [bank.xyz(i) for i in ids])
        fb.write_keypoints_dir(str(tmp_path / "kp"), ids, out["kp"], out["count"])
        for j, i in enumerate(ids):
            n = int(out["count"][j])
            b.add_fragment_result(i, out["kp"][j, :, :n].t(), out["desc"][j, :, :n].t(), clouds[i])
            kp_file = np.fromfile(str(tmp_path / "kp" / ("%d.bin" % i)), dtype=np.float32).reshape(-1, 3)
            assert np.array_equal(kp_file, out["kp"][j, :, :n].t().cpu().numpy())
    ra, rb = a.evaluate(None, scene["gt"], scene["gt_info"]), b.evaluate(None, scene["gt"], scene["gt_info"])
    assert ra["pairs"] == rb["pairs"] == 6
    assert len(ra["entries"]) == len(rb["entries"]) == ra["written"]
    for ea, eb in zip(ra["entries"], rb["entries"]):
        assert ea.info == eb.info and ea.inlier_num == eb.inlier_num and ea.inlier_ratio == eb.inlier_ratio
        assert np.array_equal(ea.trans, eb.trans) and np.array_equal(ea.information, eb.information)
    for k in ("Rt", "inliers", "inlier_ratio", "ratio_aligned", "information"):
        assert np.array_equal(ra["per_pair"][k], rb["per_pair"][k]), k
    for k in ("recall", "precision"):                            # nan where nothing passes the gate: the networks are untrained
        assert np.array_equal(np.float64(ra[k]), np.float64(rb[k]), equal_nan=True), k
    # the [xyz, descriptor] files round-trip
    for i in a.ids():
        xyz, desc = a.fragment_arrays(i)
        path = str(tmp_path / ("%d.bin" % i))
        inference.write_descriptors_bin(path, xyz, desc)
        x2, d2 = fr.read_descriptors_bin(path, D)
        assert np.array_equal(x2, xyz) and np.array_equal(d2, desc)
        assert np.array_equal(xyz, b.fragment_arrays(i)[0]) and np.array_equal(desc, b.fragment_arrays(i)[1])


def test_describe_does_not_synchronise_with_the_host(world):
    world["describer"].describe([0, 1, 3])                       # the permutation and the workspace of this size exist now
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = world["describer"].describe([3, 1, 0])
        only = world["describer"].keypoints([2, 0])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out["desc"].shape == (3, D, TOP) and only["kp"].shape == (2, 3, TOP)


def test_add_described_refuses_what_does_not_fit(world):
    from usip_amd import fragments as fr
    ev = fr.FragmentEvaluator(None, None, None, DEV, top=TOP)
    kp, desc = torch.zeros(2, 3, TOP, device=DEV), torch.zeros(2, D, TOP, device=DEV)
    count, clouds = torch.tensor([3, 4], dtype=torch.int32, device=DEV), [torch.zeros(5, 3, device=DEV)] * 2
    ev.add_described([4, 7], kp, desc, count, clouds)
    assert ev.ids() == [4, 7]
    for bad in ((kp[:1], desc, count, clouds), (kp, desc[:, :, :5], count, clouds), (kp, desc, count[:1], clouds),
                (kp, desc, count, clouds[:1])):
        with pytest.raises(ValueError):
            ev.add_described([4, 7], *bad)
    wide = torch.zeros(2, 3, TOP + 1, device=DEV)
    with pytest.raises(ValueError):
        ev.add_described([4, 7], wide, torch.zeros(2, D, TOP + 1, device=DEV), count, clouds)
