"""GPU tests of the indoor descriptor pair builder (csrc/indoor_pairs.hip): the kernels on the reference's
recorded draws, Philox mode against the host twin on every path, building into IndoorDescriptorStep's captured buffers, the
prefetched form, and IndoorDescriptorTrainer on a synthetic SceneNN-layout dataset."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_indoor_pairs_cpu import CASES, _case, check_against_fixture, fixture_frames, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(batch):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in batch.items()}


@pytest.fixture(scope="module")
def g():
    return load_golden("indoor_pairs_cases.npz")


@pytest.fixture(scope="module")
def fixture_bank(g):
    from usip_amd import indoor_pairs
    return indoor_pairs.IndoorPairBank.from_arrays(fixture_frames(g), g["pairs"], g["icp"], DEV)


@pytest.mark.parametrize("name", CASES)
def test_apply_equals_the_host_twin_and_meets_the_reference(g, fixture_bank, name):
    from usip_amd import indoor_pairs
    recipe, mode, ids, draws = _case(g, name)
    b = indoor_pairs.IndoorPairBuilder(fixture_bank, recipe, len(ids), DEV, mode=mode)
    got = _np(b.apply(ids, draws))
    rows, slots = b.last_rows.cpu().numpy(), b.last_node_slots.cpu().numpy()
    want, wrows, wslots = host(g, name)
    assert np.array_equal(rows, wrows) and np.array_equal(slots, wslots)
    for k in want:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (name, k)
    check_against_fixture(got, rows, slots, g, name, "device")


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """A SceneNN-layout dataset: 5 frames per mode, the last of 300 rows; train + val as one bank, and its host arrays."""
    from usip_amd import indoor_pairs
    root = str(tmp_path_factory.mktemp("scenenn"))
    indoor_pairs.synthetic_scenenn(root, frames=5, rows=1300, short_rows=300, seed=2)
    banks = {m: indoor_pairs.IndoorPairBank.from_root(root, m, DEV) for m in ("train", "val", "test")}
    tf, tp, ti = indoor_pairs.load_root(root, "train")
    vf, vp, vi = indoor_pairs.load_root(root, "val")
    cp, ci, cm = indoor_pairs.concat_samples(len(tf), (tp, ti, np.zeros(len(tp), np.int32)), (vp, vi, np.ones(len(vp), np.int32)))
    return dict(root=root, banks=banks, both=banks["train"] + banks["val"], host=(tf + vf, cp, ci, cm),
                test_host=indoor_pairs.load_root(root, "test"))


# (mode, P, rank, samples, (N, n_sub, M)): P = 1 and 3, both ranks, the three modes, a call mixing train and val samples
# (ids 8.. are val's), the 300-row frame as anchor (7, 15) and as positive (6, 14), and a shape that is no power of two with M no
# multiple of the workgroup
PHILOX = [("train", 1, 0, [7], (1024, 512, 32)), ("train", 3, 1, [0, 6, 3], (1024, 512, 32)),
          ("val", 3, 0, [1, 7, 6], (1024, 512, 32)), ("test", 1, 1, [6], (1024, 512, 32)),
          ("bank", 3, 1, [2, 15, 14], (1024, 512, 32)), ("bank", 3, 0, [9, 1, 7], (1000, 500, 33)),
          ("train", 1, 0, [5], (1000, 500, 33))]


@pytest.mark.parametrize("mode,P,rank,ids,shape", PHILOX)
def test_build_equals_the_host_twin_bit_for_bit(synthetic, mode, P, rank, ids, shape):
    from usip_amd import indoor_pairs
    N, n_sub, M = shape
    recipe = indoor_pairs.IndoorPairRecipe(N=N, M=M, n_sub=n_sub, translation_perturbation=int(rank == 1))
    frames, pairs, icp, modes = synthetic["host"]
    bank = synthetic["both"]
    assert bank.num_samples == 16 and bank.mode_host.tolist() == [0] * 8 + [1] * 8 and bank.min_rows == 300
    b = indoor_pairs.IndoorPairBuilder(bank, recipe, P, DEV, seed=77, rank=rank, mode=mode)
    got = _np(b.build(ids, 13, with_indices=True))
    want, wrows, wslots = indoor_pairs.build_cpu(recipe, frames, pairs, icp, ids, P, seed=77, step=13, rank=rank, mode=mode,
                                                 sample_mode=modes)
    assert np.array_equal(b.last_rows.cpu().numpy(), wrows) and np.array_equal(b.last_node_slots.cpu().numpy(), wslots)
    for k in want:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (mode, k)
    assert np.isfinite(got["anc_pc"]).all() and np.isfinite(got["pos_node"]).all()


def test_bank_from_root_thins_test_and_refuses_on_the_device_too(synthetic):
    from usip_amd import indoor_pairs
    test = synthetic["banks"]["test"]
    assert test.num_samples == 3 and test.mode_host.tolist() == [2, 2, 2]
    frames, pairs, icp = synthetic["test_host"]
    assert test.num_scans == len(frames) and np.array_equal(test.pairs_host, pairs)
    same = indoor_pairs.IndoorPairBank.from_device_rows([torch.from_numpy(f).to(DEV) for f in frames], pairs, icp, mode="test")
    assert torch.equal(same.rows, test.rows) and torch.equal(same.icp, test.icp) and torch.equal(same.pairs, test.pairs)
    bad = icp.copy()
    bad[0, 3, 1] = 0.5
    with pytest.raises(ValueError, match="last row"):
        indoor_pairs.IndoorPairBank.from_arrays(frames, pairs, bad, DEV)
    with pytest.raises(ValueError, match="names frame"):
        indoor_pairs.IndoorPairBank.from_arrays(frames, pairs + 1, icp, DEV)
    with pytest.raises(ValueError):
        indoor_pairs.IndoorPairBank.from_arrays(frames + [np.zeros((0, 7), np.float32)], pairs, icp, DEV)
    with pytest.raises(ValueError, match="columns"):
        indoor_pairs.IndoorPairBuilder(test, indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512, Cs=5), 1, DEV)
    b = indoor_pairs.IndoorPairBuilder(test, indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512), 1, DEV, mode="test")
    with pytest.raises(ValueError, match="out of range"):
        b.build([3], 0)


def _small(synthetic, graph=False, with_optimizer=True, P=2):
    """Builder and trainer at 1024 points and 32 nodes over the train + val bank, a seeded (not trained) frozen detector."""
    from usip_amd import indoor_pairs, synth
    from usip_amd.networks import IndoorOptions, build_detector
    # CGF_radius 1 m: the untrained detector's 32 keypoints of a 6 m slab lie about a metre apart, so anchors have positives;
    # sigma_max 5: its sigmas are all above the indoor 0.5, which would weight every triplet with 0
    opt = IndoorOptions(input_pc_num=1024, node_num=32, descriptor_len=64, node_knn_k_1=16, batch_size=P, CGF_radius=1.0,
                        sigma_max=5.0)
    recipe = indoor_pairs.IndoorPairRecipe.scenenn(opt)
    assert (recipe.N, recipe.n_sub, recipe.M, recipe.Cs) == (1024, 512, 32, 4)
    b = indoor_pairs.IndoorPairBuilder(synthetic["both"], recipe, P, DEV, seed=4, mode="bank")
    det = build_detector("ball", opt)
    sd = det.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    state = {k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in filled.items()}
    tr = indoor_pairs.IndoorDescriptorTrainer(b, "ball", state, opt, DEV, seed=3, graph=graph, with_optimizer=with_optimizer)
    return b, tr, recipe


SCHEDULE = [([k % 16, (k + 9) % 16], k) for k in range(4)]


def test_prefetch_gives_the_sequential_batches_and_may_be_left_early(synthetic):
    from usip_amd import indoor_pairs
    recipe = indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512)
    b = indoor_pairs.IndoorPairBuilder(synthetic["both"], recipe, 2, DEV, seed=6, mode="bank")
    seen = [{k: v.clone() for k, v in batch.items()} for batch in b.prefetch(SCHEDULE[:3])]
    assert len(seen) == 3
    for (ids, step), got in zip(SCHEDULE, seen):
        want = b.build(ids, step)
        for k in indoor_pairs.KEYS:
            assert torch.equal(got[k], want[k]), (step, k)
    outs = [indoor_pairs.empty_batch(b.c, 2, DEV) for _ in range(2)]
    torch.cuda.synchronize()
    gen = b.prefetch(SCHEDULE, outs=outs)
    for batch in gen:
        break
    del batch
    gen.close()
    for o in outs:                                       # reuse of the caller's buffers, ordered after the pending build
        for t in o.values():
            t.fill_(7)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for o in outs for t in o.values())
    want = b.build(*SCHEDULE[1])                         # and the builder still builds what it built before
    again = [x for x in b.prefetch([SCHEDULE[1]])][0]
    assert all(torch.equal(want[k], again[k]) for k in indoor_pairs.KEYS)


def _run(synthetic, graph, steps=4):
    b, tr, _ = _small(synthetic, graph=graph)
    losses = [tr.train_step(b.build(ids, step), epoch=0).detach().clone() for ids, step in SCHEDULE[:steps]]
    torch.cuda.synchronize()
    return tr, losses, {k: v.detach().clone() for k, v in tr.st.descriptor.state_dict().items()}


def test_trainer_steps_are_reproducible_eagerly_and_from_a_captured_graph(synthetic):
    """Two seeds-equal eager runs give the same losses and parameters bit for bit; so does a run that captures its third
    call and replays it (what tests/test_indoor_head_gpu.py promises of IndoorDescriptorStep itself)."""
    _, la, sa = _run(synthetic, False)
    _, lb, sb = _run(synthetic, False)
    tr, lc, sc = _run(synthetic, True)
    assert tr.st.use_graph and len(tr.st._graphs) == 1
    print("losses", [float(x) for x in la], "active", float(tr.last_active))
    assert all(bool(torch.isfinite(x)) and float(x) > 0.0 for x in la)
    for other_l, other_s in ((lb, sb), (lc, sc)):
        assert all(torch.equal(x, y) for x, y in zip(la, other_l))
        assert all(torch.equal(sa[k], other_s[k]) for k in sa)
    assert not torch.equal(la[0], la[1])


def test_build_into_the_steps_static_batch_writes_in_place_and_allocates_nothing(synthetic):
    b, tr, recipe = _small(synthetic, graph=True, with_optimizer=False)
    for ids, step in SCHEDULE[:3]:                       # calls 1-2 eager, call 3 captures
        tr.train_step(b.build(ids, step), epoch=0)
    fresh = tr.descriptor_batch({k: v.clone() for k, v in b.build([2, 11], 9).items()})
    static = tr.st.static_batch(fresh)
    assert static is not None
    from usip_amd import indoor_pairs
    shared = [k for k in indoor_pairs.KEYS if k in static]
    assert set(shared) == set(indoor_pairs.KEYS) - {"anc_node", "pos_node"}
    nodes = {k: torch.empty_like(fresh_k) for k, fresh_k in b.build([2, 11], 9).items() if k.endswith("_node")}
    out = dict({k: static[k] for k in shared}, **nodes)
    ids = b._ids([2, 11])
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    inplace = b.build(ids, 9, out=out)
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before          # every key given: nothing allocated
    assert all(inplace[k].data_ptr() == out[k].data_ptr() for k in indoor_pairs.KEYS)
    want = b.build([2, 11], 9)
    assert all(torch.equal(inplace[k], want[k]) for k in indoor_pairs.KEYS)
    fed = dict(fresh)
    fed.update({k: inplace[k] for k in shared})
    replayed = tr.st.step(fed).detach().clone()          # the replay reads what the builder wrote, with no copy in between
    torch.cuda.synchronize()
    assert bool(torch.isfinite(replayed))


def test_test_pass_and_the_checkpoint(synthetic, tmp_path):
    from usip_amd import indoor_pairs
    from usip_amd.networks import DescriptorLiteOldGlobal
    b, tr, recipe = _small(synthetic)
    tester = indoor_pairs.IndoorPairBuilder(synthetic["banks"]["test"], recipe, 1, DEV, seed=5, mode="test")
    before = {k: v.detach().clone() for k, v in tr.st.descriptor.state_dict().items()}
    loss, active = tr.test_pass(tester, [([i], i) for i in range(3)])
    assert math.isfinite(loss) and 0.0 <= active <= 1.0
    assert tr.st.descriptor.training                      # back in the mode it was found in
    assert all(torch.equal(before[k], v) for k, v in tr.st.descriptor.state_dict().items())
    path = str(tmp_path / "d.pth")
    assert tr.save_if_best(path, loss, epoch=0) and os.path.exists(path)
    sd = torch.load(path, map_location="cpu")
    assert len(sd) == 46
    DescriptorLiteOldGlobal(tr.opt).load_state_dict(sd, strict=True)
    os.remove(path)
    assert not tr.save_if_best(path, loss + 1.0, epoch=1) and not os.path.exists(path)
    assert tr.save_if_best(path, loss + 1.0, epoch=10)    # the reference also saves every tenth epoch
