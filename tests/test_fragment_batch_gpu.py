"""GPU tests of the evaluation fragment builder (csrc/fragment_batch.hip): the kernels on the reference's
recorded draws, Philox mode against the host twin at every batch size and shape the stage treats differently, the rows a
call may not write, and the bank made from a scene directory."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_fragment_batch_cpu import CASES, check_against_fixture, fixture_draws, fixture_frames, fixture_recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(batch):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in batch.items()}


@pytest.fixture(scope="module")
def g():
    return load_golden("fragment_batch_cases.npz")


@pytest.fixture(scope="module")
def bank(g):
    from usip_amd import fragment_batch as fb
    return fb.FragmentScanBank.from_arrays(fixture_frames(g), DEV)


@pytest.mark.parametrize("name", CASES)
def test_apply_equals_the_fixture_bit_for_bit(g, bank, name):
    from usip_amd import fragment_batch as fb
    b = fb.FragmentBatchBuilder(bank, fixture_recipe(g))
    got = _np(b.apply(g[name + "_ids"], fixture_draws(g, name)))
    check_against_fixture(got, b.last_rows.cpu().numpy(), b.last_node_slots.cpu().numpy(), g, name, "device")


# (ids, (N, n_sub, M)): B = 1, 2, 3 and 5; the 300-row fragment (3) alone, as the repeated last cloud of an odd batch and in
# the middle; repeated ids; a shape that is no power of two with M no multiple of the wavefront
PHILOX = [([0], (1024, 512, 32)), ([3], (1024, 512, 32)), ([1, 2], (1024, 512, 32)), ([0, 2, 3], (1024, 512, 32)),
          ([2, 3, 1, 0, 3], (1024, 512, 32)), ([2, 2], (1024, 512, 32)), ([1, 1, 1], (1000, 500, 33)),
          ([3], (1000, 500, 33)), ([0, 3, 2, 1, 0], (1000, 500, 33))]


@pytest.mark.parametrize("ids,shape", PHILOX)
def test_build_equals_the_host_twin_bit_for_bit(g, bank, ids, shape):
    from usip_amd import fragment_batch as fb
    N, n_sub, M = shape
    recipe = fb.FragmentBatchRecipe(N=N, M=M, Cs=4, n_sub=n_sub)
    b = fb.FragmentBatchBuilder(bank, recipe, seed=77)
    got = _np(b.build(ids, 13, with_indices=True))
    want, wrows, wslots = fb.build_cpu(recipe, fixture_frames(g), ids, seed=77, step=13)
    assert np.array_equal(b.last_rows.cpu().numpy(), wrows) and np.array_equal(b.last_node_slots.cpu().numpy(), wslots)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].shape[0] == len(ids)
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (ids, k)


def test_a_fragment_gets_the_same_points_whatever_batch_it_rides_in(g, bank):
    from usip_amd import fragment_batch as fb
    b = fb.FragmentBatchBuilder(bank, fixture_recipe(g), seed=11)
    three = _np(b.build([0, 2, 1], 4))
    one = _np(b.build([2], 4))
    two = _np(b.build(torch.tensor([2, 2], dtype=torch.int32, device=DEV), 4))           # ids already on the device
    for k in one:
        assert np.array_equal(three[k][1], one[k][0]) and np.array_equal(two[k][0], one[k][0]), k
        assert np.array_equal(two[k][1], one[k][0]), k


def test_an_odd_batch_writes_its_own_buffers_only(g, bank):
    """B = 3 into buffers of 4 clouds set between two guard tensors from one allocation: the fourth row is the repeated last
    fragment, and nothing either side of the buffers changes."""
    from usip_amd import fragment_batch as fb, ops
    recipe = fixture_recipe(g)
    b = fb.FragmentBatchBuilder(bank, recipe, seed=3)
    shapes = ops.fragment_batch_shapes(b.c, 3)
    assert shapes["pc"] == (4, 3, recipe.N) and shapes["node"] == (4, 3, recipe.M)
    sizes = {k: int(np.prod(s)) for k, s in shapes.items()}
    guard = 4096
    slab = torch.full((sum(sizes.values()) + guard * (len(sizes) + 1),), float("nan"), dtype=torch.float32, device=DEV)
    out, pos = {}, guard
    for k in ("pc", "sn", "node"):
        out[k] = slab[pos:pos + sizes[k]].view(shapes[k])
        pos += sizes[k] + guard
    got = b.build([1, 0, 3], 0, out=out)
    torch.cuda.synchronize()
    pos = 0
    for k in ("pc", "sn", "node"):
        assert bool(torch.isnan(slab[pos:pos + guard]).all()), "written before " + k
        pos += guard
        assert not bool(torch.isnan(slab[pos:pos + sizes[k]]).any())
        pos += sizes[k]
        assert got[k].shape[0] == 3 and got[k].data_ptr() == out[k].data_ptr()
        assert torch.equal(out[k][3], out[k][2])                                        # the phantom repeats the last fragment
    assert bool(torch.isnan(slab[pos:]).all())


def test_refusals_on_the_device_path(g, bank):
    from usip_amd import fragment_batch as fb, ops
    recipe = fixture_recipe(g)
    b = fb.FragmentBatchBuilder(bank, recipe)
    for ids in ([4], [-1], []):
        with pytest.raises(ValueError):
            b.build(ids)
    with pytest.raises(ValueError):
        fb.FragmentBatchBuilder(bank, fb.FragmentBatchRecipe(N=1024, M=32, Cs=5, n_sub=512))
    with pytest.raises(RuntimeError):
        fb.FragmentBatchBuilder(bank, fb.FragmentBatchRecipe(N=1024, M=600, Cs=4, n_sub=512))
    # the library's own checks, past the wrapper's: an id out of range in the host copy, an empty fragment, a set flag
    ids = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = {k: torch.empty(s, dtype=torch.float32, device=DEV) for k, s in ops.fragment_batch_shapes(b.c, 2).items()}
    ws = torch.empty(ops.fragment_batch_workspace_bytes(b.c, 2), dtype=torch.uint8, device=DEV)
    ops.fragment_batch_build(b.c, bank.c_dict(), ids, np.array([0, 1], np.int32), 0, 0, out, ws)
    with pytest.raises(RuntimeError, match="USIP_EINVAL"):
        ops.fragment_batch_build(b.c, bank.c_dict(), ids, np.array([0, 4], np.int32), 0, 0, out, ws)
    with pytest.raises(RuntimeError, match="USIP_EINVAL"):
        ops.fragment_batch_build(b.c, dict(bank.c_dict(), min_rows=0), ids, None, 0, 0, out, ws)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.fragment_batch_build(b.c, bank.c_dict(), ids, None, 0, 0, out, ws[:-256])
    with pytest.raises(RuntimeError):
        ops.fragment_batch_build(b.c, bank.c_dict(), ids, None, 0, 0, dict(out, pc=out["pc"][:1]), ws)


@pytest.mark.parametrize("form", ("cloud_bin_%d.npy", "%d.npy"))
def test_bank_from_a_scene_dir(tmp_path, g, form):
    """Seven-column files are uploaded as they are; xyz(id) is the device cloud of the file."""
    from usip_amd import fragment_batch as fb
    frames = fixture_frames(g)
    for i, n in ((10, 0), (2, 1), (0, 2)):
        np.save(str(tmp_path / (form % i)), frames[n])
    bank = fb.FragmentScanBank.from_scene_dir(str(tmp_path), DEV)
    assert bank.fragment_ids == [0, 2, 10] and bank.num_scans == 3 and bank.row_len == 7 and bank.min_rows == 700
    for pos, n in enumerate((2, 1, 0)):
        assert np.array_equal(bank.xyz(pos).cpu().numpy(), frames[n][:, :3])
    b = fb.FragmentBatchBuilder(bank, fixture_recipe(g), seed=1)
    got = _np(b.build([2], 0))
    want, _, _ = fb.build_cpu(fixture_recipe(g), [frames[2], frames[1], frames[0]], [2], seed=1)
    assert np.array_equal(got["pc"], want["pc"]) and np.array_equal(got["node"], want["node"])


def test_xyz_only_files_get_normals_on_the_device(tmp_path, g):
    """Three-column files: normals and curvature from prepare.ScanPreparer.normals (k = 9, viewpoint at the origin, no grid
    average): unit normals flipped about the origin, on the rows of the file in the file's order."""
    from usip_amd import fragment_batch as fb
    from usip_amd.prepare import ScanPreparer
    xyz = fixture_frames(g)[1][:, :3] + np.array([0.0, 5.0, 0.0], np.float32)
    np.save(str(tmp_path / "0.npy"), xyz)
    np.save(str(tmp_path / "1.npy"), xyz[:400])
    bank = fb.FragmentScanBank.from_scene_dir(str(tmp_path), DEV)
    assert bank.row_len == 7 and bank.lengths.tolist() == [1100, 400]
    rows = bank.rows[:1100].cpu().numpy()
    assert np.array_equal(rows[:, :3], xyz)
    nrm = rows[:, 3:6].astype(np.float64)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    c = np.abs(nrm).argmax(axis=1)                              # findPointNormals' dirLargest flip about the viewpoint (0, 0, 0)
    at = np.arange(len(c))
    assert (nrm[at, c] * xyz.astype(np.float64)[at, c] <= 0).all()
    xyzi = torch.from_numpy(np.concatenate([xyz, np.zeros((1100, 1), np.float32)], 1)).to(DEV)
    want, _ = ScanPreparer(DEV, k=9, viewpoint=(0.0, 0.0, 0.0)).normals(xyzi)
    assert np.array_equal(rows[:, 3:7], want.to(torch.float32).cpu().numpy())
