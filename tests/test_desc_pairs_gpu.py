"""GPU tests of the descriptor pair builder (csrc/desc_pairs.hip): the kernels on the reference's recorded
draws, Philox mode against the host twin at the reference's default shape, FPS nodes against the oracle, the prefetched
form, the builder feeding DescriptorStep in place (eager against graph replay), the trainer's reproducibility and the
example end to end."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_desc_pairs_cpu import CASES, CLOUD_KEYS, DESCRIPTOR_PINS, _case, check_against_fixture, fixture_bank
from test_pairs_cpu import check_device_against_twin, cs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_KEYS = CLOUD_KEYS + ("anc_pose", "pos_pose", "anc_seq", "pos_id", "neg_idx", "neg_fail")


def _np(batch):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in batch.items()}


def _bank(sequences, n):
    from usip_amd import desc_pairs
    return desc_pairs.PosedScanBank.from_sequences(sequences, DEV, min_points=n)


@pytest.mark.parametrize("name", CASES)
def test_apply_matches_reference_loader(name):
    from usip_amd import desc_pairs
    g = load_golden("desc_pairs_cases.npz")
    recipe, train, ids, draws = _case(g, name)
    scans, poses, seq = fixture_bank(g)
    bank = desc_pairs.PosedScanBank(scans, poses, seq, DEV, min_points=recipe.N)
    b = desc_pairs.DescriptorPairBuilder(bank, recipe, len(ids), DEV, mode="train" if train else "test")
    got = _np(b.apply(ids, draws))
    check_against_fixture(g, name, got, b.last_rows.cpu().numpy(), b.last_node_slots.cpu().numpy())


def _within_ulp(a, b):
    """test_pairs_gpu._within_ulp: one unit in the last place of the larger magnitude."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def test_philox_mode_matches_host_twin_at_the_reference_shape():
    from usip_amd import desc_pairs
    P = 8
    opt = types.SimpleNamespace(input_pc_num=16384, node_num=256, surface_normal_len=4, rot_perturbation=True,
                                translation_perturbation=True)
    recipe = desc_pairs.DescriptorPairRecipe.kitti(opt)
    assert (recipe.N, recipe.M, recipe.n_sub) == (16384, 256, 4096)
    seqs = desc_pairs.synthetic_sequences(2, 12, 20480, 0.8, seed=11)
    scans = [s for q in seqs for s in seqs[q][0]]
    poses = np.concatenate([seqs[q][1] for q in seqs])
    seq = [q for q in seqs for _ in seqs[q][0]]
    ids = [7, 3, 12, 5, 23, 1, 18, 6]
    b = desc_pairs.DescriptorPairBuilder(_bank(seqs, recipe.N), recipe, P, DEV, seed=123, rank=2)
    got = _np(b.build(ids, 41, with_indices=True))
    want, wrows, wslots = desc_pairs.build_cpu(recipe, scans, poses, seq, ids, P, seed=123, step=41, rank=2)
    assert np.array_equal(b.last_rows.cpu().numpy(), wrows)
    assert np.array_equal(b.last_node_slots.cpu().numpy(), wslots)
    for k in ("pos_id", "neg_idx", "neg_fail", "anc_seq", "anc_pose", "pos_pose"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert not np.array_equal(got["pos_id"], np.asarray(ids))             # somebody moved off the anchor
    for k in CLOUD_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32
        assert _within_ulp(got[k], want[k]), (k, np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize("name,mode", DESCRIPTOR_PINS)
def test_device_matches_host_twin_at_the_pinned_cases(name, mode):
    """The descriptor case of tests/golden/cloud_stage_parent_bits.npz (N = 300: two point workgroups, the second partial,
    M = 7) through the merged cloud stage's kernels: pos_id, neg_idx, rows and node slots equal, floats within one ulp."""
    check_device_against_twin(name, mode, cs.device(name, mode, DEV), cs.host_twin(name, mode), _within_ulp)


def test_nodes_are_fps_of_the_built_candidates():
    from oracle import postproc
    from usip_amd import desc_pairs
    recipe = desc_pairs.DescriptorPairRecipe(N=4096, M=128, Cs=4, n_sub=1024)
    b = desc_pairs.DescriptorPairBuilder(_bank(desc_pairs.synthetic_sequences(2, 6, 5000, 0.8, seed=5), 4096), recipe, 3,
                                         DEV, seed=9, mode="test")
    out = _np(b.build([0, 7, 11], 0))
    cand, first = (t.cpu().numpy() for t in b.workspace_candidates())
    for p in range(3):                                   # test mode: the clouds are un-augmented
        for c, side in enumerate(("anc", "pos")):
            q = c * 3 + p
            idx = postproc.fps_indices(cand[q].T.copy(), int(first[q]), recipe.M)
            assert np.array_equal(out[side + "_node"][p], cand[q][:, idx]), (side, p)


def _small(P=4, graph=False, with_optimizer=True, seed=4, mode="train"):
    """A small bank, builder and trainer: N = 2048, 64 keypoints, a seeded (not trained) frozen detector."""
    from usip_amd import desc_pairs, synth
    from usip_amd.networks import DetectorOptions, build_detector
    opt = DetectorOptions(surface_normal_len=4, node_knn_k_1=16, input_pc_num=2048, node_num=64)
    recipe = desc_pairs.DescriptorPairRecipe.kitti(opt)
    bank = _bank(desc_pairs.synthetic_sequences(2, 10, 2500, 0.8, seed=8), recipe.N)
    b = desc_pairs.DescriptorPairBuilder(bank, recipe, P, DEV, seed=seed, mode=mode)
    det = build_detector("ball", opt)
    sd = det.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    state = {k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in filled.items()}
    tr = desc_pairs.DescriptorTrainer(b, "ball", state, opt, DEV, seed=3, graph=graph, with_optimizer=with_optimizer)
    return b, tr


SCHEDULE = [([k % 20, (k + 11) % 20, (k + 5) % 20, (k + 14) % 20], k) for k in range(5)]


def test_prefetch_gives_the_sequential_batches():
    b, tr = _small()
    seen = []
    for batch in b.prefetch(SCHEDULE):
        tr.train_step(batch)                             # the consumer's work overlaps the next build
        seen.append({k: v.clone() for k, v in batch.items()})
    assert len(seen) == 5
    for (ids, step), got in zip(SCHEDULE, seen):
        want = b.build(ids, step)
        for k in ALL_KEYS:
            assert torch.equal(got[k], want[k]), (step, k)
    torch.cuda.synchronize()
    assert int(tr.neg_fail_total) == 0 and bool(torch.isfinite(tr.last_loss))


def test_prefetch_left_early_orders_the_pending_build():
    """Breaking out of prefetch leaves build k+1 in flight on the side stream (at this shape its FPS alone runs for
    milliseconds).  Closing the generator must order the current stream behind it: the caller's buffers, reused right
    after the break, keep what is written into them; so do tensors the allocator hands out again."""
    from usip_amd import desc_pairs
    recipe = desc_pairs.DescriptorPairRecipe()            # N 16384, M 256, n_sub 4096
    b = desc_pairs.DescriptorPairBuilder(_bank(desc_pairs.synthetic_sequences(2, 4, 20480, 0.8, seed=13), recipe.N),
                                         recipe, 8, DEV, seed=2)
    ids = [0, 1, 2, 3, 4, 5, 6, 7]
    outs = [desc_pairs.empty_batch(b.c, 8, DEV) for _ in range(2)]
    torch.cuda.synchronize()
    gen = b.prefetch([(ids, k) for k in range(4)], outs=outs)
    for batch in gen:
        break
    del batch
    gen.close()
    for o in outs:                                       # reuse of the caller's buffers, ordered after the pending build
        for t in o.values():
            t.fill_(7)
    torch.cuda.synchronize()
    for o in outs:
        for k, t in o.items():
            assert bool((t == 7).all()), k
    gen = b.prefetch([(ids, k) for k in range(4)])       # the builder's own buffers: dropped, handed out again
    for batch in gen:
        break
    del batch, gen
    fills = [desc_pairs.empty_batch(b.c, 8, DEV) for _ in range(2)]
    for f in fills:
        for t in f.values():
            t.fill_(7)
    torch.cuda.synchronize()
    for f in fills:
        for k, t in f.items():
            assert bool((t == 7).all()), k
    want = b.build(ids, 1)                                # and the builder still builds what it built before
    again = [x for x in b.prefetch([(ids, 1)])][0]
    assert all(torch.equal(want[k], again[k]) for k in ALL_KEYS)


def test_static_batch_fed_in_place_eager_equals_graph_replay():
    """The builder writes anc_pc / pos_pc / anc_sn / pos_sn / neg_idx of DescriptorStep's captured input buffers in
    place; the loss of the replayed graph equals the loss of the same batch run eagerly."""
    b, tr = _small(graph=True, with_optimizer=False)
    for ids, step in SCHEDULE[:3]:                       # calls 1-2 eager, call 3 captures
        tr.train_step(b.build(ids, step))
    ids = [2, 13, 7, 19]
    fresh = tr.descriptor_batch({k: v.clone() for k, v in b.build(ids, 17).items()})
    static = tr.st.static_batch(fresh)
    assert static is not None
    shared = ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "neg_idx")
    inplace = b.build(ids, 17, out={k: static[k] for k in shared})
    assert all(inplace[k].data_ptr() == static[k].data_ptr() for k in shared)
    fed = dict(fresh)
    fed.update({k: inplace[k] for k in shared})
    replayed = tr.st.step(fed).detach().clone()
    desc_r = tr.st.last["descriptors"].detach().clone()
    eager = tr.st.step(fresh, eager=True).detach().clone()
    desc_e = tr.st.last["descriptors"].detach().clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(replayed)) and torch.equal(replayed, eager) and torch.equal(desc_r, desc_e)


def test_three_trainer_steps_are_reproducible_bit_for_bit():
    runs = []
    for _ in range(2):
        b, tr = _small()
        losses = [tr.train_step(b.build(ids, step)).detach().clone() for ids, step in SCHEDULE[:3]]
        torch.cuda.synchronize()
        runs.append((losses, {k: v.detach().clone() for k, v in tr.st.descriptor.state_dict().items()}))
    (la, sa), (lb, sb) = runs
    assert all(bool(torch.isfinite(x)) for x in la)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not torch.equal(la[0], la[1])


def test_test_pass_gates_the_checkpoint(tmp_path):
    b, tr = _small()
    tester, _ = _small(mode="test", seed=5)
    before = {k: v.detach().clone() for k, v in tr.st.descriptor.state_dict().items()}
    loss, active = tr.test_pass(tester, SCHEDULE[:2])
    assert math.isfinite(loss) and 0.0 <= active <= 1.0
    assert tr.st.descriptor.training                      # back in the mode it was found in
    assert all(torch.equal(before[k], v) for k, v in tr.st.descriptor.state_dict().items())   # no_grad, eval: no change
    path = str(tmp_path / "d.pth")
    assert tr.save_if_best(path, loss) and os.path.exists(path)
    os.remove(path)
    assert not tr.save_if_best(path, loss + 1.0) and not os.path.exists(path)


def test_bank_and_argument_checks():
    from usip_amd import desc_pairs, ops
    seqs = desc_pairs.synthetic_sequences(2, 3, 1500, 0.8, seed=6)
    scans = [s for q in seqs for s in seqs[q][0]]
    poses = np.concatenate([seqs[q][1] for q in seqs])
    short = list(scans)
    short[4] = short[4][:900]
    with pytest.raises(ValueError, match=r"scan 4 \(900 rows\)"):
        desc_pairs.PosedScanBank(short, poses, [0, 0, 0, 1, 1, 1], DEV, min_points=1024)
    with pytest.raises(ValueError, match="not contiguous"):
        desc_pairs.PosedScanBank(scans, poses, [0, 1, 0, 1, 0, 1], DEV, min_points=1024)
    bank = desc_pairs.PosedScanBank(scans, poses, [0, 0, 0, 1, 1, 1], DEV, min_points=1024)
    same = desc_pairs.PosedScanBank.from_device_rows([torch.from_numpy(s).to(DEV) for s in scans], poses,
                                                     [0, 0, 0, 1, 1, 1], min_points=1024)
    assert torch.equal(bank.rows, same.rows) and torch.equal(bank.poses, same.poses)
    assert np.array_equal(bank.seq_start_host, [0, 3, 6]) and np.array_equal(same.seq_of_host, [0, 0, 0, 1, 1, 1])
    recipe = desc_pairs.DescriptorPairRecipe(N=1024, M=32, Cs=4, n_sub=256)
    with pytest.raises(ValueError, match="2 pairs"):
        desc_pairs.DescriptorPairBuilder(bank, recipe, 1, DEV)
    with pytest.raises(ValueError, match="at least N"):
        desc_pairs.DescriptorPairBuilder(bank, desc_pairs.DescriptorPairRecipe(N=2048, M=32, Cs=4, n_sub=512), 2, DEV)
    b = desc_pairs.DescriptorPairBuilder(bank, recipe, 2, DEV)
    out = desc_pairs.empty_batch(b.c, 2, DEV)
    ids = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    bad = torch.empty((2, 2, 31), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="node_slots"):
        ops.desc_pairs_build(b.c, bank.c_dict(), ids, 0, 0, 0, out, b._ws[0], None, bad)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.desc_pairs_build(b.c, bank.c_dict(), ids, 0, 0, 0, out, b._ws[0][:64])
    broken = dict(bank.c_dict(), seq_start_host=np.array([0, 4, 3], dtype=np.int32))
    with pytest.raises(RuntimeError, match="EINVAL"):
        ops.desc_pairs_build(b.c, broken, ids, 0, 0, 0, out, b._ws[0])


def test_example_trains_and_saves_a_loadable_descriptor(tmp_path):
    """examples/train_descriptor_scans.py --make-synthetic end to end at tiny shapes: a short detector run, the descriptor
    trained on built batches, finite losses, neg_fail 0 (two sequences: a candidate always exists), and a checkpoint
    that loads into DescriptorLiteOld."""
    from usip_amd import inference
    from usip_amd.networks import DescriptorLiteOld, DetectorOptions
    out = tmp_path / "descriptor.pth"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_descriptor_scans.py"), "--make-synthetic",
           str(tmp_path / "seqs"), "--synthetic-rows", "2500", "--n", "2048", "--m", "64", "--pairs", "4",
           "--detector-steps", "6", "--steps", "12", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("step", "test"))]
    assert len(lines) >= 3, r.stdout
    for ln in lines:
        assert math.isfinite(float(ln[ln.index("loss") + 1])), ln
        assert int(ln[ln.index("neg_fail") + 1]) == 0, ln
    assert r.stdout.rstrip().endswith("saved %s" % out)
    opt = DetectorOptions(surface_normal_len=4, node_knn_k_1=16, input_pc_num=2048, node_num=64)
    net = inference.load_detector_state(DescriptorLiteOld(opt), torch.load(str(out), map_location="cpu"))
    assert all(bool(torch.isfinite(v).all()) for v in net.state_dict().values())
