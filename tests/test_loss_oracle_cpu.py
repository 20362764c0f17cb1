"""CPU tests of tests/loss_oracle.py: what entitles the GPU tests of the loss kernels (test_loss_kernels_gpu.py) to use it
as the checker.  The float64 references reproduce the outputs the reference project recorded in
tests/golden/losses_cases.npz; the two 3-D references agree where both apply; the chunking rule the GPU cases are placed by
is the library's own."""
import numpy as np
import pytest
import torch

import loss_oracle as lo
from conftest import assert_close, load_golden
from oracle import detector as od


def test_chamfer_references_reproduce_the_reference_projects_fixture():
    """chamfer_f64 (on the minima) and chamfer_module_f64 (on the clouds) against pc_* of losses_cases.npz: the loss, pure,
    weighted and the four gradients at 1e-5; the minima and arg-minima fed to them are nearest_torch's."""
    g = load_golden("losses_cases.npz")
    src, dst, ss, sd = g["pc_src"], g["pc_dst"], g["pc_ss"], g["pc_sd"]
    a, J = lo.nearest_torch(src, dst)
    c, I = lo.nearest_torch(dst, src)
    r = lo.chamfer_f64(a, J, c, I, ss, sd, 1.0)
    m = lo.chamfer_module_f64(src, dst, ss, sd, J, I)
    for ref in (r, m):
        assert_close(ref["loss"], g["pc_loss"], name="loss")
        assert_close(ref["pure"], g["pc_pure"], name="pure")
        assert_close(ref["weighted"], g["pc_weighted"], name="weighted")
    assert_close(r["dss"], g["pc_gss"], name="dss")
    assert_close(r["dsd"], g["pc_gsd"], name="dsd")
    for key, want in (("gsrc", "pc_gsrc"), ("gdst", "pc_gdst"), ("gss", "pc_gss"), ("gsd", "pc_gsd")):
        assert_close(m[key], g[want], name=key)
    # da, dc of the sigma arithmetic chained with the distance's own gradient are the cloud gradients of the fixture
    ga, gb, _, _ = lo.nearest_backward_f64(src, dst, J, r["da"])
    ha, hb, _, _ = lo.nearest_backward_f64(dst, src, I, r["dc"])
    assert_close(ga + hb, g["pc_gsrc"], name="gsrc by parts")
    assert_close(gb + ha, g["pc_gdst"], name="gdst by parts")
    # the magnitudes are sums of magnitudes: never below the values they bound
    assert r["loss_mag"] >= abs(r["loss"])
    assert (r["H_ss"] >= np.abs(r["dss"]) * (1 - 1e-12)).all() and (r["H_sd"] >= np.abs(r["dsd"]) * (1 - 1e-12)).all()
    assert int(r["n_sd"].sum()) == J.size and int(r["n_ss"].sum()) == I.size


def test_nearest_references_reproduce_the_reference_projects_fixture():
    """ss_d bit for bit (nearest_torch), within the derived bound (nearest_f64), and ss_gkp (nearest_backward_f64,
    single_side_f64), which holds a keypoint ON a cloud point: a zero row of the gradient."""
    g = load_golden("losses_cases.npz")
    kp, pc, gd = g["ss_kp"], g["ss_pc"], g["ss_gd"]
    d, arg = lo.nearest_torch(kp, pc)
    assert np.array_equal(d, g["ss_d"])
    d64 = lo.nearest_f64(kp, pc)
    val, idx = lo.nearest_nd_bounds(3)
    assert (np.abs(d - d64.min(axis=2)) <= val * d64.min(axis=2)).all()
    picked = np.take_along_axis(d64, arg[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    assert (picked <= d64.min(axis=2) * (1 + idx)).all()
    ga, gb, n, S = lo.nearest_backward_f64(kp, pc, arg, gd)
    assert_close(ga, g["ss_gkp"], name="ss_gkp")
    assert float(d[0, 0]) == 0.0 and not ga[0, :, 0].any()
    d2, ga2 = lo.single_side_f64(kp, pc, arg, gd)
    assert_close(d2, g["ss_d"], name="ss_d")
    assert np.array_equal(ga2, ga)
    assert int(n.sum()) == arg.size and np.isclose(S.sum(), np.abs(gd).sum())
    for bi in range(kp.shape[0]):                      # gb is minus the segment sum
        for j in np.unique(arg[bi])[:5]:
            assert np.allclose(gb[bi, :, j], -ga[bi][:, arg[bi] == j].sum(axis=1), rtol=1e-12, atol=0)
    assert not gb[:, :, np.setdiff1d(np.arange(pc.shape[2]), arg[0])][0].any()


def test_the_two_3d_references_agree_on_a_lattice():
    """exact integers + numpy's sqrt against torch.norm + torch.min, value and first index bit for bit, on a lattice where
    more than a third of the minima are tied; and one cloud at a time equals the whole batch at once"""
    a, b = lo.cloud_lattice(3, 2, 37, 5000)
    d, arg, tied = lo.nearest_exact_lattice(a, b)
    assert tied.mean() >= lo.TIE_SHARE
    dt, argt = lo.nearest_torch(a, b)
    assert np.array_equal(d, dt) and np.array_equal(arg, argt)
    whole_d, whole_arg = torch.min(od.pairwise_norm(torch.from_numpy(a), torch.from_numpy(b)), dim=2)
    assert np.array_equal(dt, whole_d.numpy()) and np.array_equal(argt, whole_arg.numpy())
    ra, rb = lo.cloud_random(4, 3, 33, 700)
    dr, argr = lo.nearest_torch(ra, rb)
    whole_d, whole_arg = torch.min(od.pairwise_norm(torch.from_numpy(ra), torch.from_numpy(rb)), dim=2)
    assert np.array_equal(dr, whole_d.numpy()) and np.array_equal(argr, whole_arg.numpy())


def test_rolled_clouds_carry_torchs_own_answer():
    """cloud_random_rolled (the 64-cloud case of the GPU tests) against nearest_torch run on every cloud"""
    a, b, d, arg = lo.cloud_random_rolled(9, 7, 13, 300, base=2)
    want_d, want_arg = lo.nearest_torch(a, b)
    assert np.array_equal(d, want_d) and np.array_equal(arg, want_arg)
    assert not np.array_equal(a[0], a[2]) and not np.array_equal(b[1], b[3]) and not np.array_equal(arg[0], arg[2])


def test_the_lattice_reference_is_within_the_float64_bounds_for_descriptors():
    """nearest_exact_lattice against nearest_f64 at C = 7 and 131: the same value to one rounding, the same FIRST index
    (float64 is exact on these integers too), ties in more than a third of the queries"""
    for C, Nb in ((7, 65), (131, 300)):
        a, b = lo.desc_lattice(C, 2, C, 9, Nb)
        d, arg, tied = lo.nearest_exact_lattice(a, b)
        assert tied.mean() >= lo.TIE_SHARE
        d64 = lo.nearest_f64(a, b)
        assert np.array_equal(arg, np.argmin(d64, axis=2))
        assert (np.abs(d - d64.min(axis=2)) <= lo.U * d64.min(axis=2)).all()
    a, b = lo.desc_unit(5, 2, 33, 5, 70)
    assert np.allclose(np.linalg.norm(a, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(b, axis=1), 1, atol=1e-6)


def test_a_lattice_builder_refuses_an_easy_input():
    with pytest.raises(AssertionError, match="tied minimum"):
        fine = np.random.default_rng(1).integers(-512, 513, (2, 1, 3, 50)) / 64.0    # a lattice far finer than the cloud
        lo._assert_tied(fine[0, :, :, :20].astype(np.float32), fine[1].astype(np.float32))
    with pytest.raises(AssertionError, match="exact integers"):       # float32(0.1) is dyadic, but its square needs 48 bits
        lo.nearest_exact_lattice(np.full((1, 3, 1), np.float32(0.1)), np.zeros((1, 3, 2), np.float32))


# (B, Ma, Nb) -> (chunks, chunk length): the paths the GPU cases of test_loss_kernels_gpu.py exist for
CHUNK_PLANS = {
    (1, 5, 32769): (32, 1088),         # chunk 31 starts at 33728, past the end: empty
    (1, 5, 33729): (32, 1088),         # chunk 31 holds exactly one candidate
    (1, 16, 2048): (2, 1024),
    (1, 16, 2047): (1, 2047),
    (64, 256, 4096): (1, 4096),        # 1024 groups of 16 queries: one launch
    (63, 256, 4096): (2, 2048),
    (3, 33, 5000): (4, 1280),
    (1, 5, 5000): (4, 1280),           # the hand-placed cases
    (2, 1, 1): (1, 1), (1, 3, 63): (1, 63), (1, 17, 65): (1, 65), (2, 4, 257): (1, 257),
    (2, 1, 700): (1, 700), (2, 513, 40): (1, 40),      # the module cases
}


@pytest.mark.parametrize("shape", sorted(CHUNK_PLANS))
def test_chunk_plan_is_the_librarys_own(shape):
    """usip_nearest_workspace gives the chunk counts the GPU cases rely on, and loss_oracle.chunk_plan restates it: if the
    chunking rule changes, this says which GPU case stopped covering its path."""
    from usip_amd import _lib
    B, Ma, Nb = shape
    chunks, chunk = CHUNK_PLANS[shape]
    assert int(_lib.lib().usip_nearest_workspace(B, Ma, Nb)) == (chunks * B * Ma if chunks > 1 else 0)
    assert lo.chunk_plan(B, Ma, Nb) == (chunks, chunk)
    if chunks > 1:
        assert chunk % 64 == 0 and chunk * chunks >= Nb


def test_workspace_sizes_of_the_chunked_gpu_cases():
    from usip_amd import _lib
    ws = _lib.lib().usip_nearest_workspace
    assert [int(ws(*s)) for s in ((1, 5, 32769), (1, 16, 2048), (1, 16, 2047), (64, 256, 4096), (63, 256, 4096))] == \
        [32 * 5, 2 * 16, 0, 0, 2 * 63 * 256]
    assert 31 * 1088 > 32769 and 31 * 1088 == 33729 - 1              # the empty and the one-candidate last chunk
