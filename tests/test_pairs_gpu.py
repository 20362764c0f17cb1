"""GPU tests of the training-pair builder (csrc/pairs.hip): the kernels on the reference's recorded draws,
Philox mode against the host twin at the KITTI shape, FPS nodes against the oracle, distributions, and the builder
feeding DetectorStep in place (eager and graph replay) and through its prefetched form."""
import math
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_pairs_cpu import CASES, DETECTOR_PINS, KEYS, _case, check_against_fixture, check_device_against_twin, cs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scans(seed, rows, kind="slab:20"):
    from usip_amd import synth
    rng = np.random.default_rng(seed)
    return [np.concatenate([synth.make_cloud(rng, n, kind).T, synth.make_normals(rng, n, 5).T], 1).astype(np.float32)
            for n in rows]


def _np(batch):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in batch.items()}


@pytest.mark.parametrize("name", CASES)
def test_apply_matches_reference_loader(name):
    from usip_amd import pairs
    g = load_golden("pairs_cases.npz")
    recipe, train, scan, scans, draws = _case(g, name)
    bank = pairs.ScanBank([scans[scan]], DEV)           # (Oxford refuses a bank with a scan shorter than N)
    b = pairs.PairBuilder(bank, recipe, 1, DEV, mode="train" if train else "test")
    got = _np(b.apply([0], draws))
    rows, slots = b.last_rows.cpu().numpy(), b.last_node_slots.cpu().numpy()
    check_against_fixture(g, name, got, rows, slots)


def _within_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))))


@pytest.mark.parametrize("preset", ["kitti", "oxford"])
def test_philox_mode_matches_host_twin_at_kitti_shape(preset):
    from usip_amd import pairs
    P = 8
    opt = types.SimpleNamespace(input_pc_num=16384, node_num=512, surface_normal_len=4, rot_perturbation=True,
                                translation_perturbation=True)
    recipe = pairs.PairRecipe.kitti(opt) if preset == "kitti" else pairs.PairRecipe.oxford(opt)
    rows = [20480] * 7 + ([12000] if preset == "kitti" else [17000])    # KITTI: one scan takes the fix_idx layout
    scans = _scans(11, rows)
    ids = [7, 3, 0, 5, 7, 1, 2, 6]
    b = pairs.PairBuilder(pairs.ScanBank(scans, DEV), recipe, P, DEV, seed=123, rank=2)
    got = _np(b.build(ids, 41, with_indices=True))
    want, wrows, wslots = pairs.build_cpu(recipe, scans, ids, P, seed=123, step=41, rank=2)
    assert np.array_equal(b.last_rows.cpu().numpy(), wrows)
    assert np.array_equal(b.last_node_slots.cpu().numpy(), wslots)
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32
        assert _within_ulp(got[k], want[k]), (k, np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize("name,mode", DETECTOR_PINS)
def test_device_matches_host_twin_at_the_pinned_cases(name, mode):
    """The cases of tests/golden/cloud_stage_parent_bits.npz (N = 300: two point workgroups, the second partial; the
    fix_idx layout, Oxford's height scaling and ENU -> cam, sn_last) through the merged cloud stage's kernels."""
    check_device_against_twin(name, mode, cs.device(name, mode, DEV), cs.host_twin(name, mode), _within_ulp)


def test_nodes_are_fps_of_the_built_candidates():
    from oracle import postproc
    from usip_amd import pairs
    opt = types.SimpleNamespace(input_pc_num=4096, node_num=128, surface_normal_len=4)
    recipe = pairs.PairRecipe.kitti(opt)
    b = pairs.PairBuilder(pairs.ScanBank(_scans(5, [6000, 5000, 3000]), DEV), recipe, 3, DEV, seed=9, mode="test")
    out = _np(b.build([0, 1, 2], 0))
    cand, first = (t.cpu().numpy() for t in b.workspace_candidates())
    for p in range(3):                                   # test mode: src is the un-augmented cloud, untransformed
        idx = postproc.fps_indices(cand[p].T.copy(), int(first[p]), recipe.M)
        assert np.array_equal(out["src_node"][p], cand[p][:, idx])


def test_draw_distributions():
    """Fixed seeds; every bound is a ~1e-6 (or tighter) tail, so the test does not flake."""
    from usip_amd import pairs
    n, N, P = 100, 50, 4096
    recipe = pairs.PairRecipe(N=N, M=4, Cs=5, n_sub=16, rot_horizontal=0, aug_scale_lo=1.0, aug_scale_hi=1.0)
    scans = _scans(3, [n])
    b = pairs.PairBuilder(pairs.ScanBank(scans, DEV), recipe, P, DEV, seed=77)
    out = _np(b.build(np.zeros(P, np.int32), 3, with_indices=True))
    rows = b.last_rows.cpu().numpy().reshape(2 * P, N)
    # no duplicate source row per cloud, all in range
    assert rows.min() >= 0 and rows.max() < n
    assert all(len(np.unique(r)) == N for r in rows)
    # the first slot is uniform over [0, n): chi-square, 99 dof, P(> 200) ~ 1e-8
    cnt = np.bincount(rows[:, 0], minlength=n)
    exp = 2 * P / n
    assert ((cnt - exp) ** 2 / exp).sum() < 200
    # slot and source index uncorrelated
    j = np.broadcast_to(np.arange(N), rows.shape).ravel()
    r = np.corrcoef(j, rows.ravel())[0, 1]
    assert abs(r) < 5.0 / math.sqrt(rows.size)
    # inclusion frequency N / n: binomial(2P, 0.5) per row, 6 sigma
    inc = np.bincount(rows.ravel(), minlength=n)
    mu, sd = 2 * P * N / n, math.sqrt(2 * P * (N / n) * (1 - N / n))
    assert np.all(np.abs(inc - mu) < 6 * sd)
    # jitter: src clouds (no rotation, scale 1, no shift): pc - p and the un-rotated sn channels 3, 4
    src_rows = rows[:P]
    bank = scans[0]
    for got, want, sigma, clip in ((out["src_pc"], bank[src_rows][:, :, 0:3].transpose(0, 2, 1), 0.04, 0.12),
                                   (out["src_sn"][:, 3:5], bank[src_rows][:, :, 6:8].transpose(0, 2, 1), 0.01, 0.05)):
        jit = got.astype(np.float64) - want
        assert np.abs(jit).max() <= clip + 1e-5
        k = jit.size
        assert abs(jit.mean()) < 6 * sigma / math.sqrt(k)
        # the clip sits at 3 (pc) and 5 (sn) sigma: variance of the clipped normal
        c = clip / sigma
        pdf, tail = math.exp(-c * c / 2) / math.sqrt(2 * math.pi), math.erfc(c / math.sqrt(2))
        var = sigma ** 2 * ((1 - tail) - 2 * c * pdf + c * c * tail)
        assert abs(jit.var() / var - 1) < 6 * math.sqrt(2.0 / k) + 1e-3
    # yaw of the transform uniform over [0, 2 pi): chi-square over 16 bins, P(> 60) ~ 1e-7
    yaw = np.mod(np.arctan2(out["R"][:, 0, 2].astype(np.float64), out["R"][:, 0, 0]), 2 * math.pi)
    cnt = np.histogram(yaw, bins=16, range=(0, 2 * math.pi))[0]
    assert ((cnt - P / 16) ** 2 / (P / 16)).sum() < 60


def _step_setup(graph):
    from usip_amd import pairs
    from usip_amd.networks import DetectorOptions
    from usip_amd.step import DetectorStep
    opt = DetectorOptions(surface_normal_len=4, node_knn_k_1=16, input_pc_num=2048, node_num=64)
    recipe = pairs.PairRecipe.kitti(opt)
    b = pairs.PairBuilder(pairs.ScanBank(_scans(8, [3000, 2500, 4000], "slab:14"), DEV), recipe, 2, DEV, seed=4)
    torch.manual_seed(3)
    st = DetectorStep("ball", opt, DEV, graph=graph)
    return b, st


@pytest.mark.parametrize("graph", [False, True])
def test_step_fed_in_place_equals_fresh_batch(graph):
    b, st = _step_setup(graph)
    for k in range(3):                                   # graph: calls 1-2 eager, call 3 captures
        st.step(b.build([k % 3, (k + 1) % 3], k))
    ids = [2, 0]
    fresh = {k: v.clone() for k, v in b.build(ids, 17).items()}
    static = st.static_batch(fresh) if graph else None
    if graph:
        assert static is not None
    inplace = b.build(ids, 17, out=static)
    if graph:
        assert all(inplace[k].data_ptr() == static[k].data_ptr() for k in KEYS)
    la = st.step(inplace).detach().clone()
    ka = st.last["keypoints"].detach().clone()
    lb = st.step(fresh).detach().clone()
    kb = st.last["keypoints"].detach().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(ka, kb)


def test_prefetch_gives_the_sequential_batches():
    b, st = _step_setup(False)
    schedule = [([k % 3, (k + 2) % 3], k) for k in range(5)]
    seen = []
    for batch in b.prefetch(schedule):
        st.step(batch)                                   # the consumer's work overlaps the next build
        seen.append({k: v.clone() for k, v in batch.items()})
    assert len(seen) == 5
    for (ids, step), got in zip(schedule, seen):
        want = b.build(ids, step)
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (step, k)


def test_prefetch_left_early_orders_the_pending_build():
    """Breaking out of prefetch leaves build k+1 in flight on the side stream (at this shape its FPS alone runs for
    milliseconds).  Closing the generator must order the current stream behind it: tensors allocated and filled right
    after the break -- the allocator hands the dropped buffers out again -- keep what was written into them."""
    from usip_amd import pairs
    opt = types.SimpleNamespace(input_pc_num=16384, node_num=512, surface_normal_len=4)
    recipe = pairs.PairRecipe.kitti(opt)
    b = pairs.PairBuilder(pairs.ScanBank(_scans(13, [20480] * 4), DEV), recipe, 8, DEV, seed=2)
    torch.cuda.synchronize()
    gen = b.prefetch([([0, 1, 2, 3, 0, 1, 2, 3], k) for k in range(4)])
    for batch in gen:
        break
    del batch, gen
    fills = [pairs.empty_batch(recipe, 8, DEV) for _ in range(2)]
    for f in fills:
        for t in f.values():
            t.fill_(7.0)
    torch.cuda.synchronize()
    for f in fills:
        for k, t in f.items():
            assert bool((t == 7.0).all()), k


def test_build_during_a_live_prefetch_uses_its_own_workspace():
    b, _ = _step_setup(False)
    schedule = [([k % 3, (k + 1) % 3], k) for k in range(4)]
    seen, interleaved = [], []
    for batch in b.prefetch(schedule):
        seen.append({k: v.clone() for k, v in batch.items()})
        interleaved.append({k: v.clone() for k, v in b.build([2, 2], 50 + len(seen)).items()})
    for (ids, step), got in zip(schedule, seen):
        want = b.build(ids, step)
        assert all(torch.equal(got[k], want[k]) for k in KEYS), step
    for i, got in enumerate(interleaved):
        want = b.build([2, 2], 51 + i)
        assert all(torch.equal(got[k], want[k]) for k in KEYS), i


def test_bank_and_argument_checks():
    from usip_amd import ops, pairs
    scans = _scans(6, [1500, 1500])
    far = scans[1].copy()
    far[:, 0] += 500.0                                   # nothing of this scan lies within 40 of the sensor
    with pytest.raises(ValueError, match="scan 1"):
        pairs.ScanBank([scans[0], far], DEV, radius_threshold=40.0)
    # the radius filter runs on the values as the file holds them: float64 here, as the reference computes it
    s64 = scans[0].astype(np.float64)
    s64[0, 0], s64[0, 2] = 40.0 + 1e-12, 0.0             # outside in float64, inside once rounded to float32
    bank = pairs.ScanBank([s64], DEV, radius_threshold=40.0)
    keep = np.linalg.norm(s64[:, [0, 2]], axis=1) <= 40.0
    assert not keep[0] and bank.lengths[0] == keep.sum()
    recipe = pairs.PairRecipe(N=1024, M=32, Cs=4, n_sub=341)
    b = pairs.PairBuilder(pairs.ScanBank(scans, DEV), recipe, 2, DEV)
    out = pairs.empty_batch(recipe, 2, DEV)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    bad = torch.empty((2, 2, 31), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="node_slots"):
        ops.pairs_build(b.c, b.bank.rows, b.bank.offsets, ids, b.bank.min_rows, 0, 0, 0, out, b._ws[0], None, bad)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.pairs_build(b.c, b.bank.rows, b.bank.offsets, ids, b.bank.min_rows, 0, 0, 0, out, b._ws[0][:64])


@pytest.mark.parametrize("dataset", ["kitti", "oxford"])
def test_example_trains_and_saves_reference_keys(dataset, tmp_path):
    """examples/train_detector_scans.py --make-synthetic end to end at a small N: finite loss, a checkpoint whose key set
    is the reference's RPN_Detector_Ball's (tests/golden/reference_state_dicts.json)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    out = tmp_path / "det.pth"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_detector_scans.py"), "--make-synthetic",
           str(tmp_path / "scans"), "--synthetic-rows", "3000", "--dataset", dataset, "--n", "2048", "--m", "64",
           "--pairs", "2", "--steps", "12", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(ln.split()[3]) for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert losses and all(math.isfinite(v) for v in losses)
    ref = json.load(open(os.path.join(GOLDEN, "reference_state_dicts.json")))["RPN_Detector_Ball"]
    assert set(torch.load(str(out))) == set(ref)
