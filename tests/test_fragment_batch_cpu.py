"""CPU tests of the evaluation fragment builder: the host twin (csrc/fragment_batch_cpu.cpp, the arithmetic of
csrc/fragment_batch_math.h that the kernels run too) under the reference's recorded draws against what the reference's own
RedwoodLoader and Match3DEvalLoader computed from them (tests/golden/fragment_batch_cases.npz,
tests/golden/make_fragment_batch_golden.py); the Philox streams, the C interface, the scene directory, the example's argument
errors, and the twin under the sanitizers."""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

CASES = ("redwood", "match3d")


@pytest.fixture(scope="module")
def g():
    return load_golden("fragment_batch_cases.npz")


def fixture_frames(g):
    return [g["frame_%d" % i] for i in range(4)]


def fixture_recipe(g):
    from usip_amd import fragment_batch as fb
    return fb.FragmentBatchRecipe(N=int(g["N"]), M=int(g["M"]), Cs=int(g["Cs"]), n_sub=int(g["n_sub"]))


def fixture_draws(g, name):
    return dict(rows=g[name + "_draw_rows"].astype(np.int32), cand=g[name + "_draw_cand"].astype(np.int32),
                first=g[name + "_draw_first"])


def check_against_fixture(got, rows, slots, g, name, who):
    """The issue's bar: rows, candidates' picks equal; pc, sn and node bit-equal to the reference's loaders."""
    assert np.array_equal(rows, g[name + "_draw_rows"].astype(np.int32)), (who, name, "rows")
    assert np.array_equal(slots, g[name + "_node_slots"]), (who, name, "the FPS picks")
    for k in ("pc", "sn", "node"):
        assert got[k].dtype == np.float32 and got[k].shape == g["%s_%s" % (name, k)].shape, (who, name, k)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.int32), g["%s_%s" % (name, k)].view(np.int32)), (who, name, k)


# ---------------------------------------------------------------------------------------------------- 0: the C interface
def test_the_included_header_is_read_exported_and_laid_out_as_the_compiler_lays_it_out(tmp_path):
    """include/usip_hip_fragment_batch.h, which usip_hip.h includes after the indoor header: its three structs and five entries
    reach usip_amd._lib (INCLUDED, per header), the library exports every entry with the signature read, and sizeof and every field's offset and size
    are the host C compiler's."""
    import ctypes
    import re
    from usip_amd import _lib
    main = open(os.path.join(ROOT, "include", "usip_hip.h")).read()
    assert main.index('#include "usip_hip_indoor_pairs.h"') < main.index('#include "usip_hip_fragment_batch.h"')
    text = open(os.path.join(ROOT, "include", "usip_hip_fragment_batch.h")).read()
    declared = sorted(set(re.findall(r"\b(usip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == ["usip_fragment_batch_" + k for k in ("apply_f32", "build_f32", "build_f32_cpu", "workspace_bytes",
                                                             "workspace_offset")]
    assert list(_lib.INCLUDED) == ["usip_hip_indoor_pairs.h", "usip_hip_fragment_batch.h"]
    structs, signatures = _lib.INCLUDED["usip_hip_fragment_batch.h"]
    assert declared == sorted(signatures)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INCLUDED))
    assert not set(structs) & (set(_lib.STRUCTS) | set(_lib.STRUCTS_INCLUDED))
    lib = _lib.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (signatures[name][0], signatures[name][1]), name
    V, I, LL, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint64
    assert signatures["usip_fragment_batch_build_f32"] == ([V, V, V, V, I, U64, U64, V, V, V], I)
    assert signatures["usip_fragment_batch_apply_f32"] == ([V, V, V, V, V, I, V, V, V], I)
    assert signatures["usip_fragment_batch_build_f32_cpu"] == ([V, V, V, V, I, U64, U64, V, I], I)
    assert signatures["usip_fragment_batch_workspace_bytes"] == ([V, I], LL)
    assert signatures["usip_fragment_batch_workspace_offset"] == ([V, I, I], LL)
    mine = structs
    assert sorted(mine) == ["usip_fragment_batch_" + k for k in ("bank", "draws", "out")]
    lines, expected = [], []
    for name, cls in mine.items():
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


def test_workspace_and_recipe_refusals():
    """usip_fragment_batch_workspace_offset: the parts ascend in 256-byte steps and hold 2 ceil(B / 2) clouds; f-5's shape rules
    and every set flag among train / sn_last / height_scaling / enu_to_cam are USIP_EINVAL."""
    from usip_amd import fragment_batch as fb, ops
    c = fb.FragmentBatchRecipe(N=1000, M=33, Cs=4, n_sub=500).c_struct(7)
    for B in (1, 2, 3, 5):
        parts = [ops.fragment_batch_workspace_offset(c, B, p) for p in range(6)]
        B2 = 2 * ((B + 1) // 2)
        assert parts[0] == 0 and all(p % 256 == 0 for p in parts) and parts == sorted(parts)
        assert parts[1] >= 48 * 8 and parts[2] - parts[1] >= B2 * 3 * 500 * 4 and parts[3] - parts[2] >= B2 * 4
        assert parts[4] - parts[3] >= B2 * 33 * 4 and parts[5] - parts[4] >= B2 * 4
        assert parts[5] == ops.fragment_batch_workspace_bytes(c, B)
    assert ops.fragment_batch_workspace_bytes(c, 3) == ops.fragment_batch_workspace_bytes(c, 4)
    for field in ("train", "sn_last", "height_scaling", "enu_to_cam"):
        bad = fb.FragmentBatchRecipe(N=1000, M=33, Cs=4, n_sub=500).c_struct(7)
        setattr(bad, field, 1)
        with pytest.raises(RuntimeError):
            ops.fragment_batch_workspace_bytes(bad, 2)
    for kw in (dict(Cs=5), dict(M=501), dict(n_sub=1001), dict(N=0)):
        with pytest.raises(RuntimeError):
            ops.fragment_batch_workspace_bytes(fb.FragmentBatchRecipe(**dict(dict(N=1000, M=33, Cs=4, n_sub=500), **kw)).c_struct(7), 2)
    with pytest.raises(RuntimeError):
        ops.fragment_batch_workspace_offset(c, 2, 6)


# ---------------------------------------------------------------------------------------------------- 1: the reference
def test_fixture_meets_the_fps_condition_and_its_shapes(g):
    """The smallest relative gap between the largest running distance and the next different value, over every FPS round of
    every item the reference ran, is at least 1e-4: a float32 sampling decides every round as the reference's float64 one."""
    assert float(g["fps_min_gap"]) >= 1e-4
    assert [len(f) for f in fixture_frames(g)] == [1180, 1100, 700, 300] and all(f.shape[1] == 7 for f in fixture_frames(g))
    assert (int(g["N"]), int(g["n_sub"]), int(g["M"]), int(g["Cs"])) == (1024, 512, 32, 4)
    assert g["redwood_ids"].tolist() == [0, 1, 2, 3] and g["match3d_ids"].tolist() == [0, 1]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fragment_batch_cases.npz")) < 1 << 20
    # recomputed here from the fixture alone, in float64 as the reference samples
    worst = np.inf
    for name in CASES:
        for b, i in enumerate(g[name + "_ids"]):
            rows, cand = g[name + "_draw_rows"][b].astype(np.int64), g[name + "_draw_cand"][b].astype(np.int64)
            pts = fixture_frames(g)[i][rows][cand, :3].astype(np.float64)
            picks = [int(np.flatnonzero(cand == s)[0]) for s in g[name + "_node_slots"][b]]
            assert picks[0] == int(g[name + "_draw_first"][b])
            dist = ((pts[picks[0]] - pts) ** 2).sum(axis=1)
            for pick in picks[1:]:
                top = dist.max()
                assert dist[pick] == top
                below = dist[dist != top]
                worst = min(worst, (top - below.max()) / top)
                dist = np.minimum(dist, ((pts[pick] - pts) ** 2).sum(axis=1))
    assert worst >= 1e-4 and worst == pytest.approx(float(g["fps_min_gap"]), rel=1e-12)


@pytest.mark.parametrize("name", CASES)
def test_twin_under_the_recorded_draws_matches_the_reference(g, name):
    from usip_amd import fragment_batch as fb
    got, rows, slots = fb.build_cpu(fixture_recipe(g), fixture_frames(g), g[name + "_ids"], draws=fixture_draws(g, name))
    check_against_fixture(got, rows, slots, g, name, "host twin")
    threaded, rt, st = fb.build_cpu(fixture_recipe(g), fixture_frames(g), g[name + "_ids"], draws=fixture_draws(g, name),
                                    num_threads=3)
    check_against_fixture(threaded, rt, st, g, name, "host twin, 3 threads")


def test_short_frames_take_the_fix_idx_layout_in_the_fixture(g):
    rows = g["redwood_draw_rows"]
    assert np.array_equal(rows[2, :700], np.arange(700)) and len(set(rows[2, 700:].tolist())) == 324
    assert np.array_equal(rows[3, :900], np.tile(np.arange(300), 3)) and len(set(rows[3, 900:].tolist())) == 124


# ---------------------------------------------------------------------------------------------------- 2: Philox
def test_philox_rows_candidates_and_layout(g):
    from usip_amd import fragment_batch as fb
    frames, recipe = fixture_frames(g), fixture_recipe(g)
    got, rows, slots = fb.build_cpu(recipe, frames, [0, 1, 2, 3], seed=5)
    N = recipe.N
    for b in (0, 1):                                             # n >= N: a permutation prefix, no repeats
        assert len(set(rows[b].tolist())) == N and rows[b].min() >= 0 and rows[b].max() < len(frames[b])
        assert not np.array_equal(rows[b], np.sort(rows[b]))
    assert np.array_equal(rows[2, :700], np.arange(700)) and len(set(rows[2, 700:].tolist())) == 324
    assert np.array_equal(rows[3, :900], np.tile(np.arange(300), 3)) and len(set(rows[3, 900:].tolist())) == 124
    assert rows[2, 700:].max() < 700 and rows[3, 900:].max() < 300
    for b in range(4):
        assert len(set(slots[b].tolist())) == recipe.M and slots[b].min() >= 0 and slots[b].max() < N   # candidates are distinct slots
        f = frames[b][rows[b]]
        assert np.array_equal(got["pc"][b], f[:, :3].T) and np.array_equal(got["sn"][b], f[:, 3:7].T)    # pure gathers
        assert np.array_equal(got["node"][b], got["pc"][b][:, slots[b]])
    # all n_sub candidates are distinct: with M = n_sub FPS visits every candidate once (the 1180-row frame has no duplicate)
    full = fb.FragmentBatchRecipe(N=64, M=32, Cs=4, n_sub=32)
    _, _, s = fb.build_cpu(full, frames, [0], seed=5)
    assert len(set(s[0].tolist())) == 32
    other, _, _ = fb.build_cpu(recipe, frames, [0], seed=6)
    assert not np.array_equal(other["pc"][0], got["pc"][0])
    stepped, _, _ = fb.build_cpu(recipe, frames, [0], seed=5, step=1)
    assert not np.array_equal(stepped["pc"][0], got["pc"][0])


def test_a_fragment_gets_the_same_points_whatever_batch_it_rides_in(g):
    from usip_amd import fragment_batch as fb
    frames, recipe = fixture_frames(g), fixture_recipe(g)
    a, ra, sa = fb.build_cpu(recipe, frames, [0, 2, 1], seed=11, step=4)
    b, rb, sb = fb.build_cpu(recipe, frames, [2], seed=11, step=4)
    c, rc, sc = fb.build_cpu(recipe, frames, [2, 2], seed=11, step=4, num_threads=2)
    for k in a:
        assert np.array_equal(a[k][1], b[k][0]) and np.array_equal(c[k][0], b[k][0]) and np.array_equal(c[k][1], b[k][0]), k
    assert np.array_equal(ra[1], rb[0]) and np.array_equal(rc[1], rb[0]) and np.array_equal(sa[1], sb[0])
    assert np.array_equal(sc[0], sb[0]) and np.array_equal(sc[1], sb[0])


def test_the_four_builders_share_no_stream(g):
    """One seed, one step, one index, one frame: tags 49-51 choose other rows than the indoor pair builder's (33-40) and the
    detector builder's (1-8)."""
    from usip_amd import fragment_batch as fb, indoor_pairs, pairs
    frame = fixture_frames(g)[0]
    _, rf, _ = fb.build_cpu(fb.FragmentBatchRecipe(N=1024, M=32, n_sub=512), [frame], [0], seed=9, step=2)
    _, ri, _ = indoor_pairs.build_cpu(indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512), [frame, frame], [[0, 1]],
                                      np.eye(4)[None], [0], 1, seed=9, step=2)
    _, rp, _ = pairs.build_cpu(pairs.PairRecipe(N=1024, M=32, n_sub=512), [np.concatenate([frame, frame[:, :1]], 1)], [0], 1,
                               seed=9, step=2)
    assert not np.array_equal(rf[0], ri[0, 0]) and not np.array_equal(rf[0], rp[0, 0])


def test_every_refusal_of_the_twin(g):
    from usip_amd import fragment_batch as fb
    frames, recipe = fixture_frames(g), fixture_recipe(g)
    fb.build_cpu(recipe, frames, [3])
    for ids in ([4], [-1], []):
        with pytest.raises(ValueError):
            fb.build_cpu(recipe, frames, ids)
    with pytest.raises(ValueError, match="empty"):
        fb.build_cpu(recipe, frames[:3] + [np.zeros((0, 7), np.float32)], [0])
    with pytest.raises((ValueError, RuntimeError)):                                       # 3 + 5 sn channels > 7 columns
        fb.build_cpu(fb.FragmentBatchRecipe(N=1024, M=32, Cs=5, n_sub=512), frames, [0])
    with pytest.raises((ValueError, RuntimeError)):
        fb.build_cpu(fb.FragmentBatchRecipe(N=1024, M=600, Cs=4, n_sub=512), frames, [0])
    d = fixture_draws(g, "match3d")
    with pytest.raises(ValueError):
        fb.build_cpu(recipe, frames, [0], draws=d)                                        # draws of two fragments for one


def test_preset_and_options():
    from usip_amd import fragment_batch as fb
    from usip_amd.networks import IndoorDetectorOptions
    opt = IndoorDetectorOptions()
    assert (opt.input_pc_num, opt.node_num, opt.surface_normal_len, opt.node_knn_k_1) == (10240, 512, 4, 32)
    r = fb.FragmentBatchRecipe.match3d(opt)
    assert (r.N, r.n_sub, r.M, r.Cs) == (10240, 5120, 512, 4)
    r = fb.FragmentBatchRecipe.match3d(opt, downsample_rate=3)
    assert (r.N, r.n_sub) == (3413, 1706)


# ---------------------------------------------------------------------------------------------------- 3: the scene directory
@pytest.mark.parametrize("form", ("cloud_bin_%d.npy", "%d.npy"))
def test_scene_dir_is_read_in_numeric_order_under_both_names(tmp_path, form):
    from usip_amd import fragment_batch as fb
    rng = np.random.default_rng(3)
    want = {i: rng.standard_normal((20 + i, 7)).astype(np.float32) for i in (0, 2, 10, 1, 11)}
    for i, a in want.items():
        np.save(str(tmp_path / (form % i)), a)
    (tmp_path / "notes.txt").write_text("not a fragment")
    np.save(str(tmp_path / "extra_3.npy"), want[0])                                     # another name: not a fragment
    ids, paths = fb.scene_files(str(tmp_path))
    assert ids == [0, 1, 2, 10, 11] and [os.path.basename(p) for p in paths] == [form % i for i in ids]
    ids, arrays = fb.load_scene_dir(str(tmp_path))
    assert all(np.array_equal(a, want[i]) for i, a in zip(ids, arrays))


def test_a_fragment_under_both_names_is_refused(tmp_path):
    from usip_amd import fragment_batch as fb
    np.save(str(tmp_path / "3.npy"), np.zeros((4, 7), np.float32))
    np.save(str(tmp_path / "cloud_bin_3.npy"), np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="two names"):
        fb.scene_files(str(tmp_path))
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no cloud_bin"):
        fb.scene_files(str(empty))


# ---------------------------------------------------------------------------------------------------- 4: the example
def _example():
    spec = importlib.util.spec_from_file_location("evaluate_fragments_example", os.path.join(ROOT, "examples",
                                                                                              "evaluate_fragments.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("argv, said", [
    (["--method", "tsf", "--descriptor-method", "fpfh"], "--method tsf describes by the learned descriptor"),
    (["--detector-ckpt", "x.pth"], "--detector-ckpt needs --method tsf"),
    (["--method", "iss", "--descriptor-method", "fpfh", "--descriptor-ckpt", "x.pth"], "--descriptor-ckpt needs"),
    (["--write-keypoints", "out"], "--write-keypoints needs --method tsf"),
    (["--method", "tsf", "--descriptor-ckpt", "no-such-file.pth"], "no checkpoint at"),
    (["--method", "tsf", "--describe-batch", "0"], "--describe-batch >= 1"),
    (["--method", "tsf", "--node-num", "6000"], "--node-num"),
    (["--method", "tsf", "--detector-model", "knn"], "invalid choice"),
    (["--method", "tsf"], "give --make-synthetic DIR"),
    (["--method", "iss"], "needs --descriptor-method fpfh, shot or spin"),
])
def test_example_argument_errors(monkeypatch, capsys, argv, said):
    """Every refusal comes from argparse, before a device or a file is touched."""
    mod = _example()
    monkeypatch.setattr(sys, "argv", ["evaluate_fragments.py"] + argv)
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 2 and said in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------- 5: the sanitizer build
SANITIZE = os.path.join(ROOT, "tests", "fragment_batch_sanitize_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = shutil.which("g++") or shutil.which("clang++") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(HIPCC) or HIPCC))), "lib", "llvm", "bin", "clang++")


def test_twin_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main) over csrc/fragment_batch_cpu.cpp: random fragments shorter and longer than N and
    of one row, batches of 1 to 5 in buffers of exactly B clouds, explicit draws with indices out of range, Philox draws on
    several threads, and every refusal.  It links nothing of the package and is never loaded into Python."""
    exe = str(tmp_path / "fragment_batch_sanitize")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", SANITIZE, os.path.join(ROOT, "usip_amd", "csrc", "fragment_batch_cpu.cpp"), "-o", exe,
                    "-lpthread"], check=True, timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode()[-2000:])
    assert r.returncode == 0 and b"runtime error" not in r.stdout and b"AddressSanitizer" not in r.stdout
