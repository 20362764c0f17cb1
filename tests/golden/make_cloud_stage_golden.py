"""Bits of the two pair builders' host twins pinned at one commit: tests/golden/cloud_stage_parent_bits.npz.

The device kernels are held to the host twins (tests/test_pairs_gpu.py, tests/test_desc_pairs_gpu.py), but twin and device
share csrc/pairs_math.h and could drift together.  This fixture holds what the twins computed in Philox mode at the commit
BEFORE the detector builder's (f-5) and the descriptor builder's (f-8) per-cloud code became one cloud stage:
tests/test_pairs_cpu.py and tests/test_desc_pairs_cpu.py hold today's twins to it bit for bit, the two GPU files the device.

Inputs are not stored: they come from seeded generators (the detector's scans from usip_amd.synth as the tests build them,
the descriptor's from desc_pairs.synthetic_sequences), and the fixture holds a SHA-256 of them, so a generator that has
moved fails the test instead of moving the expectation.

Every case: input_pc_num = 300 (two point workgroups, the second partial), node_num = 7 (M < 256), rot_perturbation and
translation_perturbation on, P pairs at seed 9, step 4, rank 1, in train and in test mode.
  D-kitti   PairRecipe.kitti (n_sub 100), scans of 300 / 512 / 130 rows, ids 2 0 1: the 130-row scan takes the fix_idx
            layout (slots 0-259 two whole copies, 260-299 keyed draws)
  D-oxford  PairRecipe.oxford (n_sub 37; height scaling, ENU -> cam, require_full), scans of 300 / 512 / 301 rows
  D-sn1     surface_normal_len = 1 (sn_last), scans of 300 / 140 rows, ids 1 0
  S-kitti   DescriptorPairRecipe.kitti (n_sub 75, mining on), synthetic_sequences(2, 6, 320, 0.8, seed=11), ids 7 3 11
Float32 outputs are stored as their bit patterns, integers as they are.

    python tests/golden/make_cloud_stage_golden.py       (regenerating it moves the pin: do that only on purpose)
"""
import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "cloud_stage_parent_bits.npz")
SHARED = dict(input_pc_num=300, node_num=7, surface_normal_len=4, rot_perturbation=True, translation_perturbation=True)
SEED, STEP, RANK, SCAN_SEED = 9, 4, 1, 21
CASES = {
    "D-kitti": dict(preset="kitti", rows=[300, 512, 130], ids=[2, 0, 1], n_sub=100),
    "D-oxford": dict(preset="oxford", rows=[300, 512, 301], ids=[2, 0, 1], n_sub=37),
    "D-sn1": dict(preset="kitti", rows=[300, 140], ids=[1, 0], n_sub=100, opt=dict(surface_normal_len=1)),
    "S-kitti": dict(preset="desc", sequences=(2, 6, 320, 0.8, 11), ids=[7, 3, 11], n_sub=75),
}
MODES = ("train", "test")
IDS = [(name, mode) for name in CASES for mode in MODES]


def is_desc(name):
    return CASES[name]["preset"] == "desc"


def recipe(name):
    from usip_amd import desc_pairs, pairs
    c = CASES[name]
    opt = types.SimpleNamespace(**dict(SHARED, **c.get("opt", {})))
    r = {"kitti": pairs.PairRecipe.kitti, "oxford": pairs.PairRecipe.oxford,
         "desc": desc_pairs.DescriptorPairRecipe.kitti}[c["preset"]](opt)
    assert (r.N, r.M, r.n_sub) == (300, 7, c["n_sub"]), (name, r)
    return r


def inputs(name):
    """-> the detector's [scans], or the descriptor's (sequences, scans, poses f64 [S, 4, 4], seq labels)."""
    c = CASES[name]
    if is_desc(name):
        from usip_amd import desc_pairs
        n_seq, n, rows, spacing, seed = c["sequences"]
        seqs = desc_pairs.synthetic_sequences(n_seq, n, rows, spacing, seed=seed)
        return (seqs, [s for q in seqs for s in seqs[q][0]], np.concatenate([seqs[q][1] for q in seqs]),
                [q for q in seqs for _ in seqs[q][0]])
    from usip_amd import synth
    rng = np.random.default_rng(SCAN_SEED)
    return [np.concatenate([synth.make_cloud(rng, n, "slab:20").T, synth.make_normals(rng, n, 5).T], 1).astype(np.float32)
            for n in c["rows"]]


def digest(name):
    inp = inputs(name)
    h = hashlib.sha256()
    for a in (inp[1] + [inp[2]] if is_desc(name) else inp):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def bits(a):
    """An output as the fixture stores it: float32 as its bit pattern, everything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def collect(batch, rows, node_slots):
    """A build's (batch, rows, node_slots) as numpy -> {field: stored form}."""
    out = dict(batch, rows=rows, node_slots=node_slots)
    return {k: bits(v) for k, v in out.items()}


def host_twin(name, mode):
    from usip_amd import desc_pairs, pairs
    ids, P = CASES[name]["ids"], len(CASES[name]["ids"])
    if is_desc(name):
        _, scans, poses, seq = inputs(name)
        got = desc_pairs.build_cpu(recipe(name), scans, poses, seq, ids, P, seed=SEED, step=STEP, rank=RANK, mode=mode)
    else:
        got = pairs.build_cpu(recipe(name), inputs(name), ids, P, seed=SEED, step=STEP, rank=RANK, mode=mode)
    return collect(*got)


def device(name, mode, dev="cuda:0"):
    """The same case through the builder's build(..., with_indices=True)."""
    import torch
    from usip_amd import desc_pairs, pairs
    ids, P = CASES[name]["ids"], len(CASES[name]["ids"])
    if is_desc(name):
        bank = desc_pairs.PosedScanBank.from_sequences(inputs(name)[0], dev, min_points=300)
        b = desc_pairs.DescriptorPairBuilder(bank, recipe(name), P, dev, seed=SEED, rank=RANK, mode=mode)
    else:
        b = pairs.PairBuilder(pairs.ScanBank(inputs(name), dev), recipe(name), P, dev, seed=SEED, rank=RANK, mode=mode)
    out = b.build(ids, STEP, with_indices=True)
    torch.cuda.synchronize()
    return collect({k: v.cpu().numpy() for k, v in out.items()}, b.last_rows.cpu().numpy(), b.last_node_slots.cpu().numpy())


def key(name, mode, field):
    return "%s_%s_%s" % (name, mode, field)


def main():
    out = {}
    for name in CASES:
        out["%s_sha256" % name] = np.frombuffer(bytes.fromhex(digest(name)), np.uint8)
        for mode in MODES:
            got = host_twin(name, mode)
            for k, v in got.items():
                out[key(name, mode, k)] = v
            if is_desc(name):
                print(name, mode, "pos_id", got["pos_id"].tolist(), "neg_idx", got["neg_idx"].tolist(), "neg_fail",
                      got["neg_fail"].tolist())
            else:
                print(name, mode, "rows[0, 2, :4]", got["rows"][0, -1, :4].tolist(), "node_slots[0, 0]",
                      got["node_slots"][0, 0].tolist())
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print("wrote", PATH, "%.0f KB" % (size / 1024))
    if size > 700 * 1024:
        raise SystemExit("the fixture is larger than 700 KB (desc_pairs_cases.npz has 727 KB)")


if __name__ == "__main__":
    main()
