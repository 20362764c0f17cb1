"""CPU tests of what the four batch builders share (usip_amd.ops: CloudBatchSpec, the struct fillers, check_draws;
usip_amd.pairs.host_twin): every declaration fills every pointer of its structs, its shape table has its KEYS, and the
host twins refuse a draw that is not in the header's layout (include/usip_hip.h, usip_pairs_draws and
usip_desc_pairs_draws; usip_hip_indoor_pairs.h; usip_hip_fragment_batch.h)."""
import ctypes

import numpy as np
import pytest

import test_desc_pairs_cpu as t_desc
import test_fragment_batch_cpu as t_frag
import test_indoor_pairs_cpu as t_indoor
import test_pairs_cpu as t_pairs
from conftest import load_golden

BUILDERS = ("pairs", "desc_pairs", "indoor_pairs", "fragment_batch")
# (builder, draw): one int32 draw of each, and one float64 draw of the two whose jitters are read
SWAPS = [(b, "rows") for b in BUILDERS] + [("pairs", "jit_pc"), ("desc_pairs", "jit_pc")]


def declaration(tag):
    """-> (the builder's CloudBatchSpec, its module's KEYS, a recipe struct at N = 1024, M = 32)."""
    from usip_amd import desc_pairs, fragment_batch, indoor_pairs, ops, pairs
    return {"pairs": (ops.PAIRS, pairs.KEYS, pairs.PairRecipe(N=1024, M=32, n_sub=341).c_struct(True)),
            "desc_pairs": (ops.DESC_PAIRS, desc_pairs.KEYS,
                           desc_pairs.DescriptorPairRecipe(N=1024, M=32, n_sub=256).c_struct(True)),
            "indoor_pairs": (ops.INDOOR_PAIRS, indoor_pairs.KEYS,
                             indoor_pairs.IndoorPairRecipe(N=1024, M=32, n_sub=512).c_struct("train", 7)),
            "fragment_batch": (ops.FRAGMENT_BATCH, fragment_batch.KEYS,
                               fragment_batch.FragmentBatchRecipe(N=1024, M=32, n_sub=512).c_struct(7))}[tag]


def null_pointers(s, prefix=""):
    """The names of the pointer fields of a header struct that are NULL, nested structs and pointer arrays included."""
    for name, ct in s._fields_:
        v = getattr(s, name)
        if isinstance(v, ctypes.Structure):
            yield from null_pointers(v, prefix + name + ".")
        elif isinstance(v, ctypes.Array):
            yield from ("%s%s[%d]" % (prefix, name, i) for i, e in enumerate(v) if not e)
        elif ct is ctypes.c_void_p and not v:
            yield prefix + name


def count_pointers(s):
    return sum(count_pointers(getattr(s, n)) if isinstance(getattr(s, n), ctypes.Structure) else
               len(getattr(s, n)) if isinstance(getattr(s, n), ctypes.Array) else int(ct is ctypes.c_void_p)
               for n, ct in s._fields_)


@pytest.mark.parametrize("tag", BUILDERS)
def test_a_declaration_fills_every_pointer_of_its_structs_and_its_table_has_its_keys(tag):
    from usip_amd import ops
    spec, keys, recipe = declaration(tag)
    c = getattr(recipe, "cloud", recipe)
    n = 2
    table = ops.cloud_batch_table(spec, recipe, n)
    assert tuple(table) == tuple(keys) == tuple(spec.keys)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    out = {k: np.zeros(shape, dtype=str(dt).replace("torch.", "")) for k, (shape, dt) in table.items()}
    rows, nodes = (np.zeros(spec.index_lead(n) + (last,), dtype=np.int32) for last in (c.N, c.M))
    o = ops.out_struct(spec, ptr, out, rows, nodes)
    assert isinstance(o, spec.out_c) and count_pointers(o) >= len(keys) + 2 and list(null_pointers(o)) == []
    # two scans of five rows, one sequence, three samples: every entry any of the four banks holds, the optional ones too
    i32 = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731
    bank = dict(rows=np.zeros((10, 7), np.float32), offsets=np.array([0, 5, 10], np.int64), min_rows=5,
                poses=np.zeros((2, 4, 4)), seq_of=i32(0, 0), seq_start=i32(0, 2), seq_start_host=i32(0, 2),
                pairs=i32(0, 1, 1, 0, 0, 1).reshape(3, 2), icp=np.zeros((3, 12)), sample_mode=i32(0, 1, 2),
                pairs_host=i32(0, 1, 1, 0, 0, 1).reshape(3, 2))
    b = ops.bank_struct(spec, ptr, bank)
    if spec.bank_c is None:                             # the detector builder's bank goes as plain arguments
        assert tag == "pairs" and b is None
    else:
        assert isinstance(b, spec.bank_c) and count_pointers(b) >= 2 and list(null_pointers(b)) == []
        assert b.min_rows == 5
    draws = {k: np.zeros([3 if e is None else e for e in shape], dtype=str(spec.draws[k]).replace("torch.", ""))
             for k, shape in spec.draw_shapes(c, n).items()}
    assert set(draws) == set(spec.draws) and set(spec.required) <= set(draws)
    ops.check_draws(spec, c, n, draws, ValueError)
    d = ops.draws_struct(spec, ptr, draws)
    assert isinstance(d, spec.draws_c) and count_pointers(d) >= 3 and list(null_pointers(d)) == []
    if tag == "desc_pairs":
        assert d.T == 3


def smallest_case(tag):
    """The smallest case of the builder's fixture that has every draw (N = 1024, M = 32, P = 1; fragments B = 2):
    dict(g, recipe, mode, ids, draws)."""
    if tag == "pairs":
        g = load_golden("pairs_cases.npz")
        recipe, train, scan, scans, draws = t_pairs._case(g, "k4_train")
        return dict(g=g, recipe=recipe, mode="train" if train else "test", ids=[scan], scans=scans, draws=draws)
    if tag == "desc_pairs":
        g = load_golden("desc_pairs_cases.npz")
        recipe, train, ids, draws = t_desc._case(g, "c4_train_end")
        return dict(g=g, recipe=recipe, mode="train" if train else "test", ids=ids, draws=draws)
    if tag == "indoor_pairs":
        g = load_golden("indoor_pairs_cases.npz")
        recipe, mode, ids, draws = t_indoor._case(g, "c4_test")
        return dict(g=g, recipe=recipe, mode=mode, ids=ids, draws=draws)
    g = load_golden("fragment_batch_cases.npz")
    return dict(g=g, recipe=t_frag.fixture_recipe(g), mode="eval", ids=g["match3d_ids"], draws=t_frag.fixture_draws(g, "match3d"))


def swapped(draws, key):
    """`draws` with the first two axes of draws[key] exchanged: as many elements, another layout."""
    assert draws[key].ndim >= 2 and draws[key].shape[0] != draws[key].shape[1]
    return dict(draws, **{key: np.ascontiguousarray(np.swapaxes(draws[key], 0, 1))})


def host_twin(tag, case, draws):
    from usip_amd import desc_pairs, fragment_batch, indoor_pairs, pairs
    g, recipe, ids = case["g"], case["recipe"], case["ids"]
    if tag == "pairs":
        return pairs.build_cpu(recipe, case["scans"], ids, 1, mode=case["mode"], draws=draws)
    if tag == "desc_pairs":
        scans, poses, seq = t_desc.fixture_bank(g)
        return desc_pairs.build_cpu(recipe, scans, poses, seq, ids, len(ids), mode=case["mode"], draws=draws)
    if tag == "indoor_pairs":
        return indoor_pairs.build_cpu(recipe, t_indoor.fixture_frames(g), g["pairs"], g["icp"], ids, len(ids),
                                      mode=case["mode"], draws=draws)
    return fragment_batch.build_cpu(recipe, t_frag.fixture_frames(g), ids, draws=draws)


@pytest.mark.parametrize("tag,key", SWAPS)
def test_the_host_twin_refuses_a_draw_that_is_not_in_the_headers_layout(tag, key):
    """(2, P, ...) for (P, 2, ...), (N, B) for (B, N): the element count is the header's, so a check that does not fire
    reads nothing past an end; the call is refused all the same."""
    case = smallest_case(tag)
    assert len(case["ids"]) == (2 if tag == "fragment_batch" else 1)
    assert case["draws"][key].shape[-1 if key == "rows" else -2] == 1024
    host_twin(tag, case, case["draws"])
    with pytest.raises((ValueError, RuntimeError)):
        host_twin(tag, case, swapped(case["draws"], key))
