"""CPU tests of the descriptor pair builder: the host twin (usip_desc_pairs_build_f32_cpu,
csrc/desc_pairs_cpu.cpp) against the reference's KittiDescriptorLoader and mine_negative_sample run on recorded draws
(tests/golden/desc_pairs_cases.npz, tests/golden/make_desc_pairs_golden.py), Philox-mode determinism, the positive search
and the mining on a synthetic trajectory, and the refusals."""
import types

import numpy as np
import pytest

from conftest import load_golden
from test_pairs_cpu import check_parent_bits, cs

CLOUD_KEYS = ("anc_pc", "anc_sn", "anc_node", "pos_pc", "pos_sn", "pos_node")
CASES = ["c4_train_end", "c1_train_far", "c5_train_pert", "c4_test_mine2", "c5_test", "c1_test_mine"]
DESCRIPTOR_PINS = [i for i in cs.IDS if cs.is_desc(i[0])]


def fixture_bank(g):
    """(scans, poses, seq) of the fixture: bank scan i is base scan scan_of[i]."""
    return [g["base_%d" % k] for k in g["scan_of"]], g["poses"], g["seq"]


def _case(g, name):
    from usip_amd import desc_pairs
    Cs, train, rh, r3, pert, transl, mine = (int(v) for v in g[name + "_case"])
    opt = types.SimpleNamespace(input_pc_num=int(g["N"]), node_num=int(g["M"]), surface_normal_len=Cs,
                                rot_horizontal=bool(rh), rot_3d=bool(r3), rot_perturbation=bool(pert),
                                translation_perturbation=bool(transl), positive_radius_threshold=float(g["radii"][0]),
                                negative_radius_threshold=float(g["radii"][1]))
    recipe = desc_pairs.DescriptorPairRecipe.kitti(opt)
    recipe.mine = mine
    draws = {k[len(name) + 6:]: g[k] for k in g if k.startswith(name + "_draw_")}
    # [P][2][...] as include/usip_hip.h lays the per-cloud draws out; the jitter normals are float16-exact values
    draws = {k: (v.astype(np.float64) if v.dtype == np.float16 else v) for k, v in draws.items()}
    return recipe, bool(train), [int(i) for i in g[name + "_ids"]], draws


def check_against_fixture(g, name, got, rows, node_slots):
    """The bars of test_pairs_cpu.check_against_fixture (whose code is tied to the detector batch's keys): every index
    equal; coordinates within 4 * 2^-24 * max|p| per array (the reference's 3x3 products run through BLAS, whose
    summation order and FMA use are not ours).  Poses are the float32 rounding of the inputs: equal."""
    assert np.array_equal(got["pos_id"], g[name + "_pos_id"]), (name, got["pos_id"], g[name + "_pos_id"])
    assert np.array_equal(got["anc_seq"], g[name + "_anc_seq"]), name
    assert np.array_equal(rows.transpose(1, 0, 2), g[name + "_draw_rows"]), name
    assert np.array_equal(node_slots, g[name + "_node_slots"]), name
    for k in ("anc_pose", "pos_pose"):
        assert np.array_equal(got[k], g["%s_%s" % (name, k)]), (name, k)
    if int(g[name + "_case"][6]):
        assert np.array_equal(got["neg_idx"], g[name + "_neg_idx"]), (name, got["neg_idx"], g[name + "_neg_idx"])
        assert int(got["neg_fail"][0]) == int(g[name + "_neg_fail"]), name
    for k in CLOUD_KEYS:
        want = np.asarray(g["%s_%s" % (name, k)], dtype=np.float64)
        have = got[k].astype(np.float64)
        assert have.shape == want.shape, (name, k, have.shape, want.shape)
        bar = 4 * 2.0**-24 * max(np.abs(want).max(), 1e-30)
        err = np.abs(have - want).max()
        print("%s %s: max error %.3e, bar %.3e" % (name, k, err, bar))
        assert err <= bar, (name, k, err, bar)


def test_fixture_margin_is_recorded():
    """The generator's condition on the poses: no distance within 100x the reference-vs-float64 difference of a radius."""
    g = load_golden("desc_pairs_cases.npz")
    assert float(g["dist_min_margin"]) > 100 * float(g["dist_max_diff"]) > 0


@pytest.mark.parametrize("name", CASES)
def test_host_twin_matches_reference_loader(name):
    from usip_amd import desc_pairs
    g = load_golden("desc_pairs_cases.npz")
    recipe, train, ids, draws = _case(g, name)
    scans, poses, seq = fixture_bank(g)
    got, rows, slots = desc_pairs.build_cpu(recipe, scans, poses, seq, ids, len(ids), mode="train" if train else "test",
                                            draws=draws)
    check_against_fixture(g, name, got, rows, slots)


def trajectory(num_seq=2, n=40, rows=1100, spacing=0.8, seed=3):
    """Slab scans on straight trajectories at `spacing` metres, sequence q offset sideways."""
    from usip_amd import synth
    rng = np.random.default_rng(seed)
    base = [np.concatenate([synth.make_cloud(rng, rows + 7 * k, "slab:20").T, synth.make_normals(rng, rows + 7 * k, 5).T],
                           1).astype(np.float32) for k in range(3)]
    scans, poses, seq = [], [], []
    for q in range(num_seq):
        for i in range(n):
            P = np.eye(4)
            P[:3, 3] = [spacing * i, 30.0 * q, 0.0]
            scans.append(base[(q * n + i) % 3])
            poses.append(P)
            seq.append(q)
    return scans, np.stack(poses), np.array(seq)


RECIPE = dict(N=1024, M=32, Cs=4, n_sub=256)


def test_philox_same_counter_same_batch_and_world_size_independence():
    from usip_amd import desc_pairs
    scans, poses, seq = trajectory()
    r = desc_pairs.DescriptorPairRecipe(**RECIPE)
    ids = [3, 50, 17, 79]
    a, ra, na = desc_pairs.build_cpu(r, scans, poses, seq, ids, 4, seed=5, step=4)
    b, rb, nb = desc_pairs.build_cpu(r, scans, poses, seq, ids, 4, seed=5, step=4)
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(ra, rb) and np.array_equal(na, nb)
    c, rc, _ = desc_pairs.build_cpu(r, scans, poses, seq, ids, 4, seed=5, step=5)
    assert not np.array_equal(ra, rc) and not np.array_equal(a["anc_pc"], c["anc_pc"])
    # a pair's clouds and positive depend on its global index rank * P + p only: rank 1 of P = 2 is pairs 2, 3 of P = 4
    s, rs, ns = desc_pairs.build_cpu(r, scans, poses, seq, ids[2:], 2, seed=5, step=4, rank=1)
    assert np.array_equal(ra[:, 2:], rs) and np.array_equal(na[:, 2:], ns)
    for k in CLOUD_KEYS + ("anc_pose", "pos_pose", "pos_id", "anc_seq"):
        assert np.array_equal(a[k][2:], s[k]), k
    # the two clouds of a pair are drawn independently, each without replacement
    assert not np.array_equal(ra[0], ra[1])
    assert all(len(set(ra[c, p])) == 1024 for c in range(2) for p in range(4))


def test_positives_lie_within_the_radius_in_the_anchors_sequence():
    from usip_amd import desc_pairs
    scans, poses, seq = trajectory()
    r = desc_pairs.DescriptorPairRecipe(**RECIPE)
    chosen = set()
    for step in range(6):
        ids = np.random.default_rng(step).permutation(80)[:16]
        out, _, _ = desc_pairs.build_cpu(r, scans, poses, seq, ids, 16, seed=1, step=step)
        pos = out["pos_id"]
        assert np.array_equal(seq[pos], seq[ids]) and np.array_equal(out["anc_seq"], seq[ids])
        d = np.linalg.norm(poses[pos][:, :3, 3] - poses[ids][:, :3, 3], axis=1)
        assert d.max() < r.positive_radius
        assert np.array_equal(out["pos_pose"], poses[pos].astype(np.float32))
        chosen.update((pos - ids).tolist())
        # two sequences 30 m apart, each 31 m long: every anchor has candidates (the other sequence at least)
        assert int(out["neg_fail"][0]) == 0
        other = out["neg_idx"]
        assert np.all(other != np.arange(16))
        far = np.linalg.norm(poses[ids[other]][:, :3, 3] - poses[ids][:, :3, 3], axis=1) > r.negative_radius
        assert np.all(far | (seq[ids[other]] != seq[ids]))
    assert len(chosen) > 6 and min(chosen) < 0 < max(chosen)          # 5 m / 0.8 m: offsets -6 .. 6, both sides


def test_rows_without_a_candidate_give_zero_and_are_counted():
    from usip_amd import desc_pairs
    scans, poses, seq = trajectory(num_seq=1, n=40)                  # one sequence, 31 m long: nobody is 50 m away
    r = desc_pairs.DescriptorPairRecipe(**RECIPE)
    out, _, _ = desc_pairs.build_cpu(r, scans, poses, seq, [0, 10, 39], 3, seed=2, step=0)
    assert np.array_equal(out["neg_idx"], [0, 0, 0]) and int(out["neg_fail"][0]) == 3
    scans, poses, seq = trajectory(num_seq=1, n=80)                  # 63 m long: only 0 and 79 are 50 m apart
    out, _, _ = desc_pairs.build_cpu(r, scans, poses, seq, [0, 30, 79, 40], 4, seed=2, step=0)
    assert np.array_equal(out["neg_idx"], [2, 0, 0, 0]) and int(out["neg_fail"][0]) == 2


def test_presets_and_refusals():
    from usip_amd import desc_pairs
    opt = types.SimpleNamespace(input_pc_num=16384, node_num=256, surface_normal_len=4, rot_3d=True)
    k = desc_pairs.DescriptorPairRecipe.kitti(opt)
    assert (k.N, k.M, k.n_sub, k.aug_scale_lo, k.aug_scale_hi, k.positive_radius, k.negative_radius, k.rot_3d) == \
        (16384, 256, 4096, 0.9, 1.1, 5.0, 50.0, 1)
    scans, poses, seq = trajectory(n=5)
    r = desc_pairs.DescriptorPairRecipe(**RECIPE)
    short = list(scans)
    short[3] = short[3][:700]
    with pytest.raises(ValueError, match=r"scan 3 \(700 rows\)"):            # a short scan, by name
        desc_pairs.build_cpu(r, short, poses, seq, [0, 1], 2)
    with pytest.raises(ValueError, match="not contiguous"):                  # a sequence in two pieces
        desc_pairs.build_cpu(r, scans, poses, [0, 0, 1, 1, 0, 0, 1, 1, 1, 1], [0, 1], 2)
    with pytest.raises(RuntimeError, match="EINVAL"):                        # mining needs two anchors
        desc_pairs.build_cpu(r, scans, poses, seq, [0], 1)
    lone = desc_pairs.DescriptorPairRecipe(mine=0, **RECIPE)
    out, _, _ = desc_pairs.build_cpu(lone, scans, poses, seq, [7], 1)        # ... and is optional
    assert out["pos_id"][0] in range(5, 10)
    with pytest.raises(RuntimeError, match="EINVAL"):                        # more FPS candidates than points
        desc_pairs.build_cpu(desc_pairs.DescriptorPairRecipe(N=1024, M=32, Cs=4, n_sub=2000), scans, poses, seq, [0, 1], 2)


def test_c_entry_refuses_a_broken_sequence_table_and_short_scans():
    """The C entry itself (the Python layer never builds such arguments): seq_start not ascending, min_rows < N."""
    import ctypes
    from usip_amd import _lib, desc_pairs, ops
    r = desc_pairs.DescriptorPairRecipe(**RECIPE)
    c = r.c_struct(True)
    scans, poses, seq = trajectory(n=4)
    rows = np.ascontiguousarray(np.concatenate(scans))
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    poses = np.ascontiguousarray(poses)
    seq_of = np.ascontiguousarray(seq, dtype=np.int32)
    ids = np.array([0, 5], dtype=np.int32)
    np_dt = {"torch.float32": np.float32, "torch.int32": np.int32, "torch.int64": np.int64}
    out = {k: np.zeros(s, dtype=np_dt[str(dt)]) for k, (s, dt) in ops.desc_pairs_shapes(c, 2).items()}
    o = ops.desc_pairs_out_struct(lambda a: a.ctypes.data, out, None, None)

    def call(seq_start, min_rows):
        st = np.ascontiguousarray(seq_start, dtype=np.int32)
        b = ops.DescPairsBankC()
        b.rows, b.offsets, b.poses, b.seq_of = rows.ctypes.data, offsets.ctypes.data, poses.ctypes.data, seq_of.ctypes.data
        b.seq_start = b.seq_start_host = st.ctypes.data
        b.num_scans, b.num_seq, b.min_rows = 8, len(st) - 1, min_rows
        return _lib.lib().usip_desc_pairs_build_f32_cpu(ctypes.addressof(c), None, ctypes.addressof(b), ids.ctypes.data, 2,
                                                        1, 0, 0, ctypes.addressof(o))
    assert call([0, 4, 8], 1100) == 0
    assert call([0, 8, 4], 1100) < 0           # descending
    assert call([0, 4, 4, 8], 1100) < 0        # an empty sequence
    assert call([0, 4, 7], 1100) < 0           # does not end at num_scans
    assert call([1, 4, 8], 1100) < 0           # does not start at 0
    assert call([0, 4, 8], 1023) < 0           # min_rows < N


@pytest.mark.parametrize("name,mode", DESCRIPTOR_PINS)
def test_host_twin_gives_the_bits_pinned_before_the_cloud_stage_was_merged(name, mode):
    """tests/golden/cloud_stage_parent_bits.npz: what the f-8 twin computed before its per-cloud loop became
    csrc/cloud_stage_host.h's -- the clouds, rows and node slots, and the positive and negatives chosen on the way."""
    check_parent_bits(name, mode, cs.host_twin(name, mode), "host twin")
