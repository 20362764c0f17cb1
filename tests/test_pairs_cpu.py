"""CPU tests of the training-pair builder: the Philox header against numpy's own Philox, the keyed
bijection, determinism, and the host twin (usip_pairs_build_f32_cpu, csrc/pairs_cpu.cpp) against the reference's
KittiLoader / OxfordLoader run on recorded draws (tests/golden/pairs_cases.npz, tests/golden/make_pairs_golden.py)."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, GOLDEN)
import make_cloud_stage_golden as cs  # noqa: E402   (the cases of tests/golden/cloud_stage_parent_bits.npz and how they are stored)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = ("src_pc", "src_sn", "src_node", "dst_pc", "dst_sn", "dst_node", "R", "scale", "shift")
DETECTOR_PINS = [i for i in cs.IDS if not cs.is_desc(i[0])]


@pytest.fixture(scope="module")
def rng_probe(tmp_path_factory):
    """csrc/pairs_rng.h compiled as plain host C++ into a tiny shared library (philox block, bijection)."""
    d = tmp_path_factory.mktemp("rng")
    src = d / "probe.cpp"
    src.write_text('#include "%s"\nusing namespace usip_pairs;\n'
                   'extern "C" void block(const uint64_t* c, const uint64_t* k, uint64_t* o) { philox4x64_10(c, k, o); }\n'
                   'extern "C" void perm(const uint64_t* b, uint64_t n, uint64_t* out) {\n'
                   '  PairsPerm p; p.init(b, n); for (uint64_t j = 0; j < n; ++j) out[j] = p(j); }\n'
                   % os.path.join(ROOT, "usip_amd", "csrc", "pairs_rng.h"))
    so = d / "probe.so"
    cxx = "g++" if subprocess.run(["which", "g++"], capture_output=True).returncode == 0 else HIPCC
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", str(src), "-o", str(so)],
                   check=True, timeout=300)
    lib = ctypes.CDLL(str(so))
    lib.block.argtypes = [ctypes.c_void_p] * 3
    lib.perm.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def test_philox_matches_numpy_block_for_block(rng_probe):
    """numpy's Philox increments the counter BEFORE it generates a block: state counter c gives philox(c + 1)."""
    g = np.random.default_rng(7)
    for _ in range(6):
        key = _u64(g.integers(0, 2**63, 2, dtype=np.uint64) * 2 + 1)
        ctr = _u64(g.integers(0, 2**63, 4, dtype=np.uint64))
        bg = np.random.Philox(key=key, counter=ctr)
        want = bg.random_raw(4)
        nxt = ctr.copy()
        nxt[0] += np.uint64(1)
        got = _u64(np.zeros(4))
        rng_probe.block(nxt.ctypes.data, key.ctypes.data, got.ctypes.data)
        assert np.array_equal(got, want)
    # the carry: counter word 0 at its maximum rolls into word 1
    key = _u64([3, 4])
    bg = np.random.Philox(key=key, counter=_u64([2**64 - 1, 5, 0, 0]))
    got = _u64(np.zeros(4))
    rng_probe.block(_u64([0, 6, 0, 0]).ctypes.data, key.ctypes.data, got.ctypes.data)
    assert np.array_equal(got, bg.random_raw(4))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1000, 2048, 5461, 16384, 20480, 65537])
def test_bijection_is_a_permutation(rng_probe, n):
    for seed in (1, 2):
        b = _u64(np.random.default_rng([n, seed]).integers(0, 2**63, 4, dtype=np.uint64))
        out = _u64(np.zeros(n))
        rng_probe.perm(b.ctypes.data, n, out.ctypes.data)
        assert np.array_equal(np.sort(out), np.arange(n, dtype=np.uint64))
        if n >= 1000:
            assert not np.array_equal(out, np.arange(n, dtype=np.uint64))
            assert abs(np.corrcoef(out.astype(np.float64), np.arange(n))[0, 1]) < 0.1


def _scans(seed=3, rows=(1500, 700, 2000)):
    from usip_amd import synth
    rng = np.random.default_rng(seed)
    return [np.concatenate([synth.make_cloud(rng, n, "slab:20").T, synth.make_normals(rng, n, 5).T], 1)
            .astype(np.float32) for n in rows]


def test_same_counter_same_batch_and_step_changes_it():
    from usip_amd import pairs
    scans = _scans()
    r = pairs.PairRecipe(N=1024, M=32, Cs=4, n_sub=341)
    a, ra, na = pairs.build_cpu(r, scans, [0, 1, 2], 3, seed=5, step=4)
    b, rb, nb = pairs.build_cpu(r, scans, [0, 1, 2], 3, seed=5, step=4)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(ra, rb) and np.array_equal(na, nb)
    c, rc, _ = pairs.build_cpu(r, scans, [0, 1, 2], 3, seed=5, step=5)
    assert not np.array_equal(ra, rc) and not np.array_equal(a["R"], c["R"])
    # a pair's data depends on its global index rank * P + p only: rank 1 of P = 1 is pair 1 of rank 0 with P = 2
    w, rw, _ = pairs.build_cpu(r, scans, [0, 2], 2, seed=5, step=4)
    s, rs, _ = pairs.build_cpu(r, scans, [2], 1, seed=5, step=4, rank=1)
    assert np.array_equal(rw[:, 1], rs[:, 0])
    for k in KEYS:
        assert np.array_equal(w[k][1], s[k][0]), k
    # drawn without replacement, in range; the short scan (700 < N rows) takes the fix_idx layout
    for c in range(2):
        assert len(set(ra[c, 0])) == 1024 and ra[c, 0].max() < 1500 and ra[c, 2].max() < 2000
        assert np.array_equal(ra[c, 1, :700], np.arange(700)) and len(set(ra[c, 1, 700:])) == 324


def _case(g, name):
    from usip_amd import pairs
    kind, Cs, train, rh, r3, pert, transl, scan = (int(v) for v in g[name + "_case"])
    opt = types.SimpleNamespace(input_pc_num=int(g["N"]), node_num=int(g["M"]), surface_normal_len=Cs,
                                rot_horizontal=bool(rh), rot_3d=bool(r3), rot_perturbation=bool(pert),
                                translation_perturbation=bool(transl), is_height_scaling=True)
    recipe = pairs.PairRecipe.kitti(opt) if kind == 0 else pairs.PairRecipe.oxford(opt)
    draws = {k[len(name) + 6:]: g[k] for k in g if k.startswith(name + "_draw_")}
    draws = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in draws.items()}
    scans = [g["scan_%d" % i] for i in range(3)]
    return recipe, bool(train), scan, scans, draws


CASES = ["k1_train", "k4_train", "k5_train", "k4_test", "o4_train", "o5_train", "o5_test", "k1_norot"]


def check_against_fixture(g, name, got, rows, node_slots):
    """indices equal; coordinates within 4 * 2^-24 * max|p| per cloud (the reference's 3x3 products run through BLAS /
    torch sgemm, whose summation order and FMA use are not ours)."""
    assert np.array_equal(rows[:, 0], g[name + "_draw_rows"][0]), name
    assert np.array_equal(node_slots, g[name + "_node_slots"]), name
    for k in KEYS:
        want = np.asarray(g["%s_%s" % (name, k)], dtype=np.float64).reshape(got[k].shape[1:])
        have = got[k][0].astype(np.float64)
        bar = 4 * 2.0**-24 * max(np.abs(want).max(), 1e-30)
        err = np.abs(have - want).max()
        assert err <= bar, (name, k, err, bar)


@pytest.mark.parametrize("name", CASES)
def test_host_twin_matches_reference_loader(name):
    from usip_amd import pairs
    g = load_golden("pairs_cases.npz")
    recipe, train, scan, scans, draws = _case(g, name)
    got, rows, node_slots = pairs.build_cpu(recipe, scans, [scan], 1, mode="train" if train else "test", draws=draws)
    check_against_fixture(g, name, got, rows, node_slots)


def test_presets_and_refusals():
    from usip_amd import pairs
    opt = types.SimpleNamespace(input_pc_num=16384, node_num=512, surface_normal_len=4)
    k, o = pairs.PairRecipe.kitti(opt), pairs.PairRecipe.oxford(opt)
    assert (k.n_sub, o.n_sub, k.aug_scale_lo, o.aug_scale_hi, o.enu_to_cam, k.sn_last) == (5461, 2048, 0.9, 1.3, 1, 0)
    assert pairs.PairRecipe.kitti(types.SimpleNamespace(surface_normal_len=1)).sn_last == 1
    with pytest.raises(ValueError):
        pairs.PairRecipe.oxford(types.SimpleNamespace(surface_normal_len=1))
    scans = _scans(rows=(1500, 700))
    small = types.SimpleNamespace(input_pc_num=1024, node_num=32, surface_normal_len=4)
    with pytest.raises(RuntimeError, match="EINVAL"):            # an Oxford scan shorter than N
        pairs.build_cpu(pairs.PairRecipe.oxford(small), scans, [1], 1)
    with pytest.raises(RuntimeError, match="EINVAL"):            # FPS over more than 16384 candidates
        pairs.build_cpu(pairs.PairRecipe(N=60000, M=32, Cs=4, n_sub=20000), scans, [0], 1)
    order = pairs.epoch_order(10, 1, 0)
    assert sorted(order) == list(range(10)) and np.array_equal(order, pairs.epoch_order(10, 1, 0))
    assert not np.array_equal(order, pairs.epoch_order(10, 1, 1))
    b = list(pairs.epoch_batches(10, 2, 1, 0, rank=1, world=2))
    assert len(b) == 2 and np.array_equal(b[0], order[2:4]) and np.array_equal(b[1], order[6:8])


def check_parent_bits(name, mode, got, what):
    """Every stored output of (case, mode), bit for bit; the inputs' digest first (nothing is skipped when it moves)."""
    want = load_golden(os.path.basename(cs.PATH))
    assert bytes(want["%s_sha256" % name]).hex() == cs.digest(name), "the generators no longer give the fixture's inputs"
    stored = {k[len(cs.key(name, mode, "")):]: want[k] for k in want if k.startswith(cs.key(name, mode, ""))}
    assert set(stored) == set(got) and {"rows", "node_slots"} <= set(stored), (sorted(stored), sorted(got))
    differ = {k: int((got[k] != e).sum()) if got[k].shape == e.shape else -1 for k, e in stored.items()}
    print("%s, %s %s: entries that differ from the pinned bits %s" % (what, name, mode, differ))
    for k, e in stored.items():
        assert got[k].dtype == e.dtype and got[k].shape == e.shape, k
        assert np.array_equal(got[k], e), (what, name, mode, k, differ[k])


@pytest.mark.parametrize("name,mode", DETECTOR_PINS)
def test_host_twin_gives_the_bits_pinned_before_the_cloud_stage_was_merged(name, mode):
    """Twin and device are held together everywhere else; this holds the twin to what the f-5 twin computed before its
    per-cloud loop became csrc/cloud_stage_host.h's (the fix_idx layout, Oxford's height scaling and ENU -> cam, sn_last)."""
    check_parent_bits(name, mode, cs.host_twin(name, mode), "host twin")


def check_device_against_twin(name, mode, got, want, within_ulp):
    """A case of the fixture through build(..., with_indices=True): integer outputs equal the twin's, float outputs (stored
    as their bit patterns) lie within the GPU files' _within_ulp of it."""
    assert set(got) == set(want)
    differ = {k: int((got[k] != w).sum()) if got[k].shape == w.shape else -1 for k, w in want.items()}
    print("device, %s %s: entries that differ from the twin's %s" % (name, mode, differ))
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        if w.dtype == np.uint32:
            g, w = got[k].view(np.float32), w.view(np.float32)
            assert within_ulp(g, w), (name, mode, k, np.abs(g - w).max())
        else:
            assert np.array_equal(got[k], w), (name, mode, k)
