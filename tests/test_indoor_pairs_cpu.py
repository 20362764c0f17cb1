"""CPU tests of the indoor descriptor pair builder: the host twin (csrc/indoor_pairs_cpu.cpp, the arithmetic of
csrc/indoor_pairs_math.h that the kernels run too) under the reference's recorded draws against what the reference's own
SceneNNDescriptorLoader computed from them (tests/golden/indoor_pairs_cases.npz, tests/golden/make_indoor_pairs_golden.py);
the on-disk layout, the refusals, the Philox streams, and the twin under the sanitizers."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

CASES = ("c4_train_2dp_short", "c4_train_norot_shift", "c3_train_3d", "c4_val_p2", "c4_test")
MODE_NAMES = ("train", "val", "test")
EXACT = ("pos_pc", "pos_sn", "pos_node", "anc_R_pos", "anc_scale_pos", "anc_shift_pos")   # never through the ICP product


@pytest.fixture(scope="module")
def g():
    return load_golden("indoor_pairs_cases.npz")


def fixture_frames(g):
    return [g["frame_%d" % i] for i in range(4)]


def _case(g, name):
    """-> (recipe, mode, sample ids, draws in f-5's layouts)."""
    from usip_amd import indoor_pairs
    mode, Cs, rh, r3, pert, transl = (int(v) for v in g[name + "_case"])
    N, M = int(g["N"]), int(g["M"])
    recipe = indoor_pairs.IndoorPairRecipe(N=N, M=M, Cs=Cs, n_sub=N // 2, rot_horizontal=rh, rot_3d=r3, rot_perturbation=pert,
                                           translation_perturbation=transl)
    draws = {k: g["%s_draw_%s" % (name, k)] for k in ("rows", "cand", "first", "params")}
    return recipe, MODE_NAMES[mode], g[name + "_ids"], draws


def one_ulp(a, b):
    """|a - b| is at most one float32 unit in the last place of the larger."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


def check_against_fixture(got, rows, slots, g, name, who):
    """The bars of the issue: indices equal; what never passes through the ICP product bit-equal; the anchor's moved
    values within one float32 ulp (np.dot's summation order is BLAS's, so its last float64 bit is nobody's to promise)."""
    assert np.array_equal(rows, g[name + "_draw_rows"].astype(np.int32).transpose(1, 0, 2)), (who, name, "rows")
    assert np.array_equal(slots, g[name + "_node_slots"]), (who, name, "the FPS picks")
    for k in EXACT:
        assert np.array_equal(got[k].view(np.int32), g["%s_%s" % (name, k)].view(np.int32)), (who, name, k)
    assert np.array_equal(got["anc_sn"][:, 3:].view(np.int32), g[name + "_anc_sn"][:, 3:].view(np.int32)), (who, name)
    for k, sl in (("anc_pc", slice(None)), ("anc_node", slice(None)), ("anc_sn", slice(0, 3))):
        assert one_ulp(got[k][:, sl], g["%s_%s" % (name, k)][:, sl]), (who, name, k)


def host(g, name, **kw):
    from usip_amd import indoor_pairs
    recipe, mode, ids, draws = _case(g, name)
    for k, v in kw.pop("recipe", {}).items():
        setattr(recipe, k, v)
    return indoor_pairs.build_cpu(recipe, fixture_frames(g), g["pairs"], g["icp"], ids, len(ids), mode=mode, draws=draws, **kw)


# ---------------------------------------------------------------------------------------------------- 0: the C interface
def test_the_included_header_is_read_exported_and_laid_out_as_the_compiler_lays_it_out(tmp_path):
    """include/usip_hip_indoor_pairs.h, which usip_hip.h includes: its four structs and five entries reach usip_amd._lib beside
    the main header's (tests/test_cabi.py checks those), the library exports every entry with the signature read, and sizeof
    and every field's offset and size are the host C compiler's."""
    import ctypes
    import re
    from usip_amd import _lib
    text = open(os.path.join(ROOT, "include", "usip_hip_indoor_pairs.h")).read()
    declared = sorted(set(re.findall(r"\b(usip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(_lib.SIGNATURES_INCLUDED) and len(declared) == 5
    assert not set(declared) & set(_lib.SIGNATURES) and not set(_lib.STRUCTS_INCLUDED) & set(_lib.STRUCTS)
    lib = _lib.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (_lib.SIGNATURES_INCLUDED[name][0], _lib.SIGNATURES_INCLUDED[name][1]), name
    V, I, LL, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint64
    assert _lib.SIGNATURES_INCLUDED["usip_indoor_pairs_build_f32_cpu"] == ([V, V, V, V, I, U64, U64, LL, V, I], I)
    assert _lib.SIGNATURES_INCLUDED["usip_indoor_pairs_workspace_offset"] == ([V, I, I], LL)
    assert sorted(_lib.STRUCTS_INCLUDED) == ["usip_indoor_pairs_" + k for k in ("bank", "draws", "out", "recipe")]
    lines, expected = [], []
    for name, cls in _lib.STRUCTS_INCLUDED.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        expected.append("%s %d" % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (name, field, name, field, name, field))
            expected.append("%s.%s %d %d" % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "usip_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)]).decode().split("\n")[:-1] == expected
    assert dict(_lib.STRUCTS_INCLUDED["usip_indoor_pairs_recipe"]._fields_)["cloud"] is _lib.STRUCTS["usip_pairs_recipe"]
    assert dict(_lib.STRUCTS_INCLUDED["usip_indoor_pairs_draws"]._fields_)["cloud"] is _lib.STRUCTS["usip_pairs_draws"]


# ---------------------------------------------------------------------------------------------------- 1: the reference
def test_fixture_meets_the_fps_condition_and_its_size(g):
    assert float(g["fps_min_gap"]) >= 1e-4
    assert 0.0 <= float(g["anchor_unequal_share"]) <= 1.0
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "indoor_pairs_cases.npz"))
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "indoor_head.npz"))
    lens = [len(f) for f in fixture_frames(g)]
    assert lens == [1180, 1100, 700, 300]


@pytest.mark.parametrize("name", CASES)
def test_twin_under_the_recorded_draws_matches_the_reference(g, name):
    got, rows, slots = host(g, name)
    check_against_fixture(got, rows, slots, g, name, "host twin")


def test_short_frames_take_the_fix_idx_layout(g):
    """700 rows: one whole copy and a draw of 324; 300 rows: three copies and 124 -- the recorded rows say so, and the twin
    followed them (above)."""
    rows = g["c4_train_2dp_short_draw_rows"]
    assert np.array_equal(rows[0, 0, :700], np.arange(700)) and len(set(rows[0, 0, 700:].tolist())) == 324
    assert np.array_equal(rows[1, 1, :900], np.tile(np.arange(300), 3)) and len(set(rows[1, 1, 900:].tolist())) == 124


def test_normals_without_the_translation_against_numpy(g):
    """icp_moves_normals = 0: sn[0:3] takes the rotation part, ((m0 x + m1 y) + m2 z) in float64 rounded once; with 1 the
    reference's translation is added.  Test mode: nothing else touches the anchor.  Everything else is unchanged."""
    name = "c4_test"
    want, _, _ = host(g, name)
    got, rows, _ = host(g, name, recipe=dict(icp_moves_normals=0))
    s = int(g[name + "_ids"][0])
    m = g["icp"][s]
    n = fixture_frames(g)[int(g["pairs"][s, 0])][rows[0, 0], 3:6].astype(np.float64)
    rot = np.stack([(m[i, 0] * n[:, 0] + m[i, 1] * n[:, 1]) + m[i, 2] * n[:, 2] for i in range(3)])
    assert np.array_equal(got["anc_sn"][0, :3], rot.astype(np.float32))
    assert np.array_equal(want["anc_sn"][0, :3], (rot + m[:3, 3:4]).astype(np.float32))
    assert not np.array_equal(got["anc_sn"][0, :3], want["anc_sn"][0, :3])
    for k in want:
        if k != "anc_sn":
            assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["anc_sn"][0, 3:], want["anc_sn"][0, 3:])


def test_anchor_lands_on_the_positive_of_a_synthetic_pair(tmp_path):
    """synthetic_scenenn's icp is the true relative pose: in test mode the moved anchor and the positive, its transform
    undone, are two samples of one thin slab in one frame."""
    from usip_amd import indoor_pairs
    indoor_pairs.synthetic_scenenn(str(tmp_path), frames=3, rows=1500, seed=3, modes=("test",))
    frames, pairs, icp = indoor_pairs.load_root(str(tmp_path), "test")
    recipe = indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512)
    out, _, _ = indoor_pairs.build_cpu(recipe, frames, pairs, icp, [0], 1, seed=5, mode="test")
    R, s, t = out["anc_R_pos"][0].astype(np.float64), float(out["anc_scale_pos"][0, 0]), out["anc_shift_pos"][0]
    pos = R.T @ ((out["pos_pc"][0].astype(np.float64) - t) / s)
    # both clouds are samples of one plane: the anchor's points lie within the positive's thin extent along its normal
    centre = pos.mean(axis=1, keepdims=True)
    normal = np.linalg.svd(pos - centre)[0][:, 2]
    assert np.abs(normal @ (pos - centre)).max() < 0.3
    assert np.abs(normal @ (out["anc_pc"][0] - centre)).max() < 0.3


# ---------------------------------------------------------------------------------------------------- 2: the bank's layout
def test_layout_read_back_thinning_and_concatenation(tmp_path):
    from usip_amd import indoor_pairs
    root = str(tmp_path)
    counts = indoor_pairs.synthetic_scenenn(root, frames=5, rows=1200, short_rows=300, seed=1)
    assert counts == dict(train=8, val=8, test=8)
    with open(os.path.join(root, "info_train.pkl"), "rb") as f:
        info = pickle.load(f)
    assert info["pairs_np"].shape == (8, 2) and info["icp_np"].shape == (8, 4, 4)
    frames, pairs, icp = indoor_pairs.load_root(root, "train")
    assert [f.shape for f in frames] == [(1200, 7)] * 4 + [(300, 7)] and frames[0].dtype == np.float32
    assert np.array_equal(pairs, info["pairs_np"]) and np.array_equal(icp, info["icp_np"])
    assert np.array_equal(frames[2], np.load(os.path.join(root, "frames_train", "2.npy")))
    # mode 'test' keeps samples 0, 3, 6; only the frames those name are read, renumbered in order
    with open(os.path.join(root, "info_test.pkl"), "rb") as f:
        info = pickle.load(f)
    paths, tp, ti, used = indoor_pairs.root_layout(root, "test")
    assert np.array_equal(used[tp], info["pairs_np"][::3]) and np.array_equal(ti, info["icp_np"][::3]) and len(tp) == 3
    assert [os.path.basename(p) for p in paths] == ["%d.npy" % i for i in used]
    # train + val: val's frame ids move up, every sample keeps its mode
    vf, vp, vi = indoor_pairs.load_root(root, "val")
    cp, ci, cm = indoor_pairs.concat_samples(len(frames), (pairs, icp, np.zeros(8, np.int32)), (vp, vi, np.ones(8, np.int32)))
    assert np.array_equal(cp[:8], pairs) and np.array_equal(cp[8:], vp + 5) and np.array_equal(ci[8:], vi)
    assert cm.tolist() == [0] * 8 + [1] * 8
    # one call mixing a train and a val sample: pair p equals pair p of the call that is all train / all val
    recipe = indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512)
    args = (recipe, frames + vf, cp, ci, [1, 9], 2)
    mixed, mr, _ = indoor_pairs.build_cpu(*args, seed=7, step=3, mode="bank", sample_mode=cm)
    tr, _, _ = indoor_pairs.build_cpu(*args, seed=7, step=3, mode="train")
    va, _, _ = indoor_pairs.build_cpu(*args, seed=7, step=3, mode="val")
    for k in mixed:
        assert np.array_equal(mixed[k][0], tr[k][0]) and np.array_equal(mixed[k][1], va[k][1]), k
    assert not np.array_equal(tr["anc_pc"][1], va["anc_pc"][1])           # val: no scale
    with pytest.raises((ValueError, RuntimeError)):
        indoor_pairs.build_cpu(*args, mode="bank")                       # no sample modes to read


def test_every_refusal(g):
    from usip_amd import indoor_pairs
    frames, pairs, icp = fixture_frames(g), g["pairs"], g["icp"]
    recipe = indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512)
    ok = lambda **kw: indoor_pairs.build_cpu(kw.pop("recipe", recipe), kw.pop("frames", frames), kw.pop("pairs", pairs),   # noqa: E731
                                             kw.pop("icp", icp), [0], 1, **kw)
    ok()
    bad = icp.copy()
    bad[2, 3, 3] = 1.0 + 2.0 ** -40
    with pytest.raises(ValueError, match="last row"):
        ok(icp=bad)
    bad = icp.copy()
    bad[0, 3, 0] = 1e-300
    with pytest.raises(ValueError, match="last row"):
        ok(icp=bad)
    for frame in (4, -1):
        p = pairs.copy()
        p[3, 1] = frame
        with pytest.raises(ValueError, match="names frame"):
            ok(pairs=p)
    with pytest.raises((ValueError, RuntimeError)):                                           # 3 + 5 sn channels > 7 columns
        ok(recipe=indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512, Cs=5))
    with pytest.raises((ValueError, RuntimeError)):                                           # the ICP move needs sn[0:3]
        ok(recipe=indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512, Cs=2))
    with pytest.raises(ValueError, match="empty"):
        ok(frames=frames[:3] + [np.zeros((0, 7), np.float32)])
    with pytest.raises(ValueError):
        ok(icp=icp[:3])
    with pytest.raises((ValueError, RuntimeError)):
        indoor_pairs.build_cpu(recipe, frames, pairs, icp, [5], 1)                            # a sample that is not there
    with pytest.raises(ValueError):
        indoor_pairs.build_cpu(recipe, frames, pairs, icp, [0], 1, mode="eval")


# ---------------------------------------------------------------------------------------------------- 3: Philox
def test_a_pair_depends_on_seed_step_and_global_index_only(g):
    from usip_amd import indoor_pairs
    frames, pairs, icp = fixture_frames(g), g["pairs"], g["icp"]
    recipe = indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512, translation_perturbation=1)
    three, r3, s3 = indoor_pairs.build_cpu(recipe, frames, pairs, icp, [0, 3, 2], 3, seed=11, step=4, rank=0)
    one, r1, s1 = indoor_pairs.build_cpu(recipe, frames, pairs, icp, [2], 1, seed=11, step=4, rank=2)
    for k in one:
        assert np.array_equal(one[k][0], three[k][2]), k
    assert np.array_equal(r1[:, 0], r3[:, 2]) and np.array_equal(s1[:, 0], s3[:, 2])
    other, _, _ = indoor_pairs.build_cpu(recipe, frames, pairs, icp, [2], 1, seed=11, step=5, rank=2)
    assert not np.array_equal(other["anc_pc"], one["anc_pc"])
    threaded, rt, st = indoor_pairs.build_cpu(recipe, frames, pairs, icp, [0, 3, 2], 3, seed=11, step=4, num_threads=3)
    for k in three:
        assert np.array_equal(threaded[k], three[k]), k
    assert np.array_equal(rt, r3) and np.array_equal(st, s3)


def test_the_three_builders_share_no_stream(g):
    """One seed, one step, one pair index, frames of one length: the indoor builder (tags 33-40), the outdoor descriptor
    builder (17-26) and the detector builder (1-8) choose different rows."""
    from usip_amd import desc_pairs, indoor_pairs, pairs
    frames = fixture_frames(g)[:2]
    eight = [np.concatenate([f, f[:, :1]], 1) for f in frames]
    N, M = 1024, 32
    _, ri, _ = indoor_pairs.build_cpu(indoor_pairs.IndoorPairRecipe(N=N, M=M, n_sub=512), [frames[0], frames[0]], [[0, 1]],
                                      g["icp"][:1], [0], 1, seed=9, step=2)
    _, rp, _ = pairs.build_cpu(pairs.PairRecipe(N=N, M=M, n_sub=512), [eight[0]], [0], 1, seed=9, step=2)
    _, rd, _ = desc_pairs.build_cpu(desc_pairs.DescriptorPairRecipe(N=N, M=M, n_sub=512, mine=0), [eight[0], eight[0]],
                                    [np.eye(4), np.eye(4)], [0, 0], [0], 1, seed=9, step=2)
    for a, b in ((ri, rp), (ri, rd), (rp, rd)):
        assert not np.array_equal(a[0, 0], b[0, 0])
    assert sorted(set(ri[0, 0].tolist())) == sorted(ri[0, 0].tolist())          # still a draw without replacement


# ---------------------------------------------------------------------------------------------------- 4: the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "indoor_pairs_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/indoor_pairs_cpu.cpp: random frames shorter and longer than N, every
    mode and the per-sample one, explicit draws with indices out of range, Philox draws on several threads, and every
    refusal.  It links nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "indoor_pairs_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "indoor_pairs_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
