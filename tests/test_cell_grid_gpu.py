"""csrc/cell_grid.hip: the cell grid of a cloud and the ball query / nearest point through it.

Every comparison is bit for bit against the brute-force entry points on the same inputs (ops.ball_query_coords,
ops.nearest): torch.equal on the indices and on the bits of the distances.  The route byte of every row says whether
the grid answered or the launch scanned the row in index order; the cases state what they expect of it, since a scan
compared with a scan would prove nothing about the grid.

tests/golden/ball_query_ancestor_cases.npz holds distance matrices without coordinates, so none of its rows applies
to a coordinate query; the coordinate fixture of the suite (dist_ball_cases.npz) is compared below."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GRID, SCAN = 1, 0


def _ops():
    from usip_amd import ops
    return ops


def _clouds(kind, B, N, seed):
    from usip_amd import synth
    rng = np.random.default_rng(seed)
    return np.stack([synth.make_cloud(rng, N, kind) for _ in range(B)]).astype(F), rng


def _nodes_from(x, M, rng):
    return np.ascontiguousarray(np.stack([x[b][:, rng.permutation(x.shape[2])[:M]] for b in range(x.shape[0])]))


def _ball(x, node, r=2.0, K=64, edge=None):
    """-> (rows, route bytes, grid), after asserting the rows equal the brute-force launch's."""
    ops = _ops()
    tx, tn = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(node)).to(DEV)
    grid = ops.cell_grid_build(tx, r * ops.cell_edge_factor() if edge is None else edge,
                               ops.ball_block_limit(x.shape[2], K))            # as RPN_Detector_Ball builds it
    got, route = ops.ball_query_grid(tn, grid, r, K, with_route=True)
    want = ops.ball_query_coords(tn, tx, r, K)
    assert torch.equal(got, want), "rows differ: %s" % (got != want).any(-1).nonzero()[:8].tolist()
    return got.cpu().numpy(), route.cpu().numpy(), grid


def _nearest(x, q, edge=2.0625):
    ops = _ops()
    tx, tq = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(q)).to(DEV)
    grid = ops.cell_grid_build(tx, edge)
    d, j, route = ops.nearest_grid(tq, grid, with_route=True)
    wd, wj = ops.nearest(tq, tx)
    assert torch.equal(j, wj), "arg differs at %s" % (j != wj).nonzero()[:8].tolist()
    assert torch.equal(d.view(torch.int32), wd.view(torch.int32))
    return d.cpu().numpy(), j.cpu().numpy(), route.cpu().numpy(), grid


# ------------------------------------------------------------------ the grid itself
def test_grid_build_sorts_every_point_into_its_cell():
    x, _ = _clouds("slab:12", 3, 2048, 1)
    ops = _ops()
    grid = ops.cell_grid_build(torch.from_numpy(x).to(DEV), 2.0625)
    pts, cs = grid.pts.cpu().numpy(), grid.cell_start.cpu().numpy()
    for b, h in enumerate(grid.header()):
        assert h["usable"] and h["edge"] >= 2.0625 and np.prod(h["dim"]) <= 15360
        assert np.array_equal(np.array(h["origin"], F), x[b].min(1))
        idx = pts[b, :, 3].view(np.int32)
        assert np.array_equal(np.sort(idx), np.arange(2048))                      # a permutation of the cloud
        assert np.array_equal(pts[b, :, :3], x[b].T[idx])
        c = [np.clip(np.floor((x[b, d] - F(h["origin"][d])) * F(h["inv"])), 0, h["dim"][d] - 1).astype(int) for d in range(3)]
        cell = (c[2] * h["dim"][1] + c[1]) * h["dim"][0] + c[0]                   # fp32 arithmetic as csrc/cell_grid.h
        cells = int(np.prod(h["dim"]))
        assert cs[b, 0] == 0 and cs[b, cells] == 2048 and (np.diff(cs[b, :cells + 1]) >= 0).all()
        pos = np.empty(2048, int)
        pos[idx] = np.arange(2048)
        assert ((cs[b][cell] <= pos) & (pos < cs[b][cell + 1])).all()


# ------------------------------------------------------------------ ball query
def test_ball_sparse_slab_every_row_from_the_grid():
    """Case 1: ~45 hits per ball, below K: cyclic padding, and no row at all may fall back to the scan."""
    x, rng = _clouds("slab:12", 3, 2048, 2)
    rows, route, _ = _ball(x, _nodes_from(x, 64, rng))
    assert (route == GRID).all()
    assert (rows[:, :, 0] == rows[:, :, -1]).sum() < rows.shape[0] * rows.shape[1]      # padded rows, not constant ones


def test_ball_dense_slab_full_balls():
    """Case 2: ~400 hits per ball; the K smallest indices in order whichever route a row takes.  The build finds the
    clouds dense (27 * N / cells > sqrt(N K)), leaves them unsorted and every row scans; without that rule
    (max_block = 0) the rows reach the same decision one by one."""
    x, rng = _clouds("slab:4", 3, 2048, 3)
    node = _nodes_from(x, 64, rng)
    rows, route, grid = _ball(x, node)
    assert not any(h["usable"] for h in grid.header()) and (route == SCAN).all()
    ops = _ops()
    tx, tn = torch.from_numpy(x).to(DEV), torch.from_numpy(node).to(DEV)
    sorted_grid = ops.cell_grid_build(tx, 2.0 * ops.cell_edge_factor())
    assert all(h["usable"] for h in sorted_grid.header())
    assert torch.equal(ops.ball_query_grid(tn, sorted_grid, 2.0, 64), torch.from_numpy(rows).to(DEV))
    inside = (np.linalg.norm(node[:, :, :, None].astype(np.float64) - x[:, :, None, :], axis=1) <= 1.99).sum(-1)
    full = inside >= 64                                                                 # (nodes high above the slab are not)
    assert full.mean() > 0.8 and (np.diff(rows, axis=-1) > 0)[full].all()               # full rows ascend strictly
    # a small radius on the same cloud: few points per cell block, rows from the grid with fewer than K hits
    _, route, _ = _ball(x, _nodes_from(x, 64, rng), r=0.5)
    assert (route == GRID).any()


@pytest.mark.parametrize("K,N,M", [(8, 2048, 64), (1, 2048, 64), (64, 1001, 64), (64, 3, 64), (8, 1001, 1), (1, 3, 1)])
def test_ball_small_k_and_odd_sizes(K, N, M):
    """Case 3: K = 8 and 1, N = 1001 and 3 (no multiple of 4: the scalar scan as fallback), M = 1."""
    x, rng = _clouds("slab:12", 3, N, 4)
    node = np.ascontiguousarray(np.stack([x[b][:, rng.integers(0, N, M)] for b in range(3)]))
    _, route, _ = _ball(x, node, K=K)
    if K >= 8 and N == 1001:
        assert (route == GRID).any()


def test_ball_all_points_identical():
    """Case 4: one cell; the node on the points (a full row 0..K-1) and farther than the radius (zeros)."""
    x = np.tile(np.array([1.5, -2.0, 7.25], F).reshape(1, 3, 1), (3, 1, 2048))
    node = np.tile(np.array([1.5, -2.0, 7.25], F).reshape(1, 3, 1), (3, 1, 64))
    node[:, 0, 32:] += F(2.5)
    rows, route, grid = _ball(x, node)                # 2048 candidates in the one cell: dense, the scan's early exit is shorter
    assert all(not h["usable"] and h["dim"] == [1, 1, 1] for h in grid.header()) and (route == SCAN).all()
    assert np.array_equal(rows[:, :32], np.broadcast_to(np.arange(64), (3, 32, 64))) and not rows[:, 32:].any()
    rows, route, _ = _ball(x[:, :, :16], node)        # 16 of them: every row from the grid, the far nodes clamped into it
    assert np.array_equal(rows[:, :32], np.broadcast_to(np.arange(64) % 16, (3, 32, 64))) and not rows[:, 32:].any()
    assert (route == GRID).all()


def test_ball_points_at_the_radius_and_on_cell_borders():
    """Case 5: from the header the build kernel wrote: points exactly on cell borders and one float to either side,
    along every axis, and nodes exactly the radius away from them in both directions."""
    x, rng = _clouds("slab:12", 3, 2048, 5)
    x[:, :, 0] = np.array([-13, -5, -13], F)
    x[:, :, 1] = np.array([13, 5, 13], F)             # pins the bounding box: the origin is (-13, -5, -13)
    ops = _ops()
    hdr = ops.cell_grid_build(torch.from_numpy(x).to(DEV), 2.0 * ops.cell_edge_factor()).header()
    nodes = []
    n = 2
    for b, h in enumerate(hdr):
        assert h["origin"] == [-13.0, -5.0, -13.0] and h["usable"]
        e = F(h["edge"])
        for axis in range(3):
            for k in (1, 2, h["dim"][axis] - 1):
                border = F(h["origin"][axis]) + F(k) * e
                for v in (border, np.nextafter(border, F(-100)), np.nextafter(border, F(100))):
                    p = np.array([0.25, 0.5, -0.75], F)
                    p[axis] = v
                    for sign in (-2.0, 2.0):          # the node exactly the radius away: dx = +-2, dy = dz = 0
                        q = p.copy()
                        q[axis] = F(v + F(sign))
                        x[b, :, n] = p
                        nodes.append((b, q))
                    n += 1
    assert n < 200
    node = np.zeros((3, 3, 64), F)
    x[:, :, 200] = np.array([1.25, 0.5, -3.75], F)    # and one where the difference is exactly the radius: s = 4 <= T
    for b in range(3):
        mine = [q for bb, q in nodes if bb == b]
        assert len(mine) == 54
        node[b, :, :54] = np.array(mine).T
        for i in range(6):
            node[b, :, 54 + i] = x[b, :, 200]
            node[b, i // 2, 54 + i] += F(2.0 if i % 2 else -2.0)
    rows, route, grid = _ball(x, node)
    assert [h["origin"] for h in grid.header()] == [[-13.0, -5.0, -13.0]] * 3          # the borders are still the borders
    assert (route == GRID).all()
    assert all(200 in rows[b, 54 + i] for b in range(3) for i in range(6))
    # the suite's coordinate fixture, against its recorded rows as well
    g = load_golden("dist_ball_cases.npz")
    rows, _, _ = _ball(g["x"], g["node"], r=float(g["radius"]), K=int(g["K"]))
    assert np.array_equal(rows, g["ball_idx_unpinned"])


@pytest.mark.parametrize("r", [0.3, 1.7, 2.0])
def test_ball_radius_whose_edge_product_rounds_differently(r):
    """radius * factor in double, rounded to float, can be one float below the float product (0.3, 1.7): the kernel's own
    edge check (radius * 1.015625) must not turn that into scans."""
    x, rng = _clouds("slab:12", 3, 2048, 9)
    _, route, grid = _ball(x, _nodes_from(x, 64, rng), r=r)
    assert all(h["usable"] for h in grid.header()) and (route == GRID).all()


def test_ball_nodes_outside_the_box():
    """Case 6: nodes beyond every face of the bounding box, nearer and farther than the radius from it."""
    x, rng = _clouds("slab:12", 3, 2048, 6)
    node = _nodes_from(x, 64, rng)
    lo, hi = x.min(2), x.max(2)
    for i in range(48):
        axis, up, far = i % 3, (i // 3) % 2, (i // 6) % 2
        off = F(3.5 if far else 1.0)
        node[:, axis, i] = (hi[:, axis] + off) if up else (lo[:, axis] - off)
    node[:, :, 48] = hi + F(0.5)                      # beyond a corner
    node[:, :, 49] = lo - F(100.0)
    _, route, _ = _ball(x, node)
    assert (route == GRID).all()


def test_ball_non_finite_clouds_are_scanned():
    """Case 7: cloud 0 holds a NaN, cloud 2 an infinity: their rows say scan, cloud 1's say grid."""
    x, rng = _clouds("slab:12", 3, 2048, 7)
    node = _nodes_from(x, 64, rng)
    x[0, 1, 777] = np.nan
    x[2, 2, 5] = -np.inf
    node[1, 0, 3] = np.nan                            # a NaN node of a usable cloud: an empty row from the grid
    rows, route, grid = _ball(x, node)
    assert [h["usable"] for h in grid.header()] == [False, True, False]
    assert (route[0] == SCAN).all() and (route[2] == SCAN).all() and (route[1] == GRID).all()
    assert not rows[1, 3].any()


def test_ball_huge_extent_coarsens_the_grid():
    """Case 8: two clusters 1e6 apart: the edge grows until the cells can be counted, or the rows are scanned."""
    x, rng = _clouds("slab:12", 3, 2048, 8)
    x[:, :, 1024:] += F(1e6)
    node = _nodes_from(x, 64, rng)
    _, route, grid = _ball(x, node)
    for h in grid.header():
        assert not h["usable"] or (h["edge"] > 1000.0 and np.prod(h["dim"]) <= 15360)
    assert (route == SCAN).all()                      # ~1000 candidates per coarse cell block: beyond the rule
    # a narrower edge than the radius needs is refused on the device, row by row
    _, route, _ = _ball(x[:, :, :1024], node[:, :, :8], edge=1.0)
    assert (route == SCAN).all()


# ------------------------------------------------------------------ nearest
def test_nearest_random_queries_and_cloud_points():
    """Case 1 and the route condition: queries on cloud points (distance 0) and random ones; every query whose
    nearest point lies within one cell edge must have come from the grid."""
    x, rng = _clouds("slab:12", 3, 2048, 11)
    q = _nodes_from(x, 64, rng)
    q[:, :, 32:] += rng.normal(0, 1.0, (3, 3, 32)).astype(F)
    d, _, route, grid = _nearest(x, q)
    assert (d[:, :32] == 0).all()
    edge = np.array([h["edge"] for h in grid.header()], F)[:, None]
    assert (route[d <= edge] == GRID).all() and (route == GRID).sum() >= 3 * 60


def test_nearest_duplicates_lowest_index_wins():
    """Case 2: every point twice (and one five times, scattered over the index range)."""
    x, rng = _clouds("slab:12", 3, 1024, 12)
    perm = rng.permutation(2048)
    x = np.concatenate([x, x], 2)[:, :, perm]
    x[:, :, [1900, 40, 700, 1333, 41]] = x[:, :, [1900]]
    q = x[:, :, rng.integers(0, 2048, 64)].copy()
    q[:, :, 0] = x[:, :, 1900]
    _, j, route, _ = _nearest(x, q)
    first = [int((x[b] == x[b][:, [1900]]).all(0).argmax()) for b in range(3)]          # <= 40
    assert j[:, 0].tolist() == first and max(first) <= 40 and (route == GRID).all()


def test_nearest_squared_distances_that_tie_after_the_root():
    """Case 3 (csrc/pair_scan.h): s = 1 + 2^-23 at index 10 and s = 1 at index 1500 both have sqrt 1.0: the minimum of
    the squared distances is at 1500, the answer is index 10."""
    x, _ = _clouds("slab:12", 3, 2048, 13)
    keep = np.linalg.norm(x, axis=1) < 1.5
    x[:, 0][keep] += F(6.0)                            # nothing else near the origin
    x[:, :, 10] = np.array([1.0, 1.5 * 2.0 ** -12, 0.0], F)
    x[:, :, 1500] = np.array([1.0, 0.0, 0.0], F)
    s10 = F(F(1.0) + F(1.5 * 2.0 ** -12) ** 2)
    assert s10 == np.nextafter(F(1), F(2)) and np.sqrt(s10) == F(1.0)
    q = np.zeros((3, 3, 64), F)
    q[:, :, 1:] = x[:, :, 100:163] + F(0.125)
    d, j, route, _ = _nearest(x, q)
    assert (j[:, 0] == 10).all() and (d[:, 0] == 1.0).all() and (route[:, 0] == GRID).all()


def test_nearest_far_queries_reach_the_ring_cap():
    """Case 4: queries far outside the box (and one NaN, one infinite query) are scanned by the same launch."""
    x, rng = _clouds("slab:12", 3, 2048, 14)
    q = _nodes_from(x, 64, rng)
    q[:, 0, :16] += F(500.0)
    q[:, 1, 16:24] -= F(40.0)
    q[:, 2, 24] = np.nan
    q[:, 0, 25] = np.inf
    _, _, route, _ = _nearest(x, q)
    assert (route[:, :26] == SCAN).all() and (route[:, 26:] == GRID).all()


def test_nearest_non_finite_clouds_are_scanned():
    """Case 5."""
    x, rng = _clouds("slab:12", 3, 2048, 15)
    q = _nodes_from(x, 64, rng)
    x[0, 0, 2047] = np.nan
    x[2, 1, 0] = np.inf
    _, _, route, _ = _nearest(x, q)
    assert (route[0] == SCAN).all() and (route[2] == SCAN).all() and (route[1] == GRID).all()


def test_nearest_single_point_cloud():
    """Case 6: N = 1; one cell, every query finds it through the grid."""
    x, rng = _clouds("slab:12", 3, 1, 16)
    q = rng.normal(0, 5, (3, 3, 64)).astype(F)
    _, j, route, _ = _nearest(x, q)
    assert not j.any() and (route == GRID).all()


# ------------------------------------------------------------------ whole step
def test_detector_step_is_the_same_with_and_without_the_grid(monkeypatch):
    """DetectorStep("ball") with the grid and with the switch off (ops.CELL_GRID is what USIP_CELL_GRID=0 sets when
    the package is imported): eager, then graph replay for three steps with Adam.  Every tensor of st.last, every index
    tensor and every parameter must be equal bit for bit."""
    from usip_amd import ops, synth
    from usip_amd.networks import DetectorOptions
    from usip_amd.step import DetectorStep, batch_to_device
    opt = DetectorOptions(surface_normal_len=4, node_knn_k_1=8)
    batches = [batch_to_device(synth.make_pair_batch(60 + i, 2, 2048, 64, 4, "slab:14"), DEV) for i in range(5)]

    def run(flag, graph):
        monkeypatch.setattr(ops, "CELL_GRID", flag)
        torch.manual_seed(9)
        st = DetectorStep("ball", opt, DEV, with_optimizer=True, graph=graph)
        seen = []
        for b in batches:                              # graph: calls 1-2 eager, 3 captures and replays, 4-5 replay
            st.step(b)
            assert st.detector.last_grid is None       # taken by the step (or never built)
            seen.append({k: v.detach().clone() for k, v in list(st.last.items()) + list(st.detector.last_indices.items())})
        return seen, {k: v.detach().clone() for k, v in st.detector.state_dict().items()}

    # the comparison is grid against scan: at this size the step's own two searches are answered by the grid
    b0 = batches[0]
    pc, node = torch.cat((b0["src_pc"], b0["dst_pc"]), 0), torch.cat((b0["src_node"], b0["dst_node"]), 0).contiguous()
    grid = ops.cell_grid_build(pc.contiguous(), 2 * ops.cell_edge_factor(), ops.ball_block_limit(2048, 64))
    assert all(h["usable"] for h in grid.header())
    assert (ops.ball_query_grid(node, grid, 2, 64, with_route=True)[1] == GRID).all()
    kp = run(True, False)[0][0]["keypoints"].contiguous()
    assert float((ops.nearest_grid(kp, grid, with_route=True)[2] == GRID).float().mean()) > 0.9

    for graph in (False, True):
        (on, p_on), (off, p_off) = run(True, graph), run(False, graph)
        for i, (a, b) in enumerate(zip(on, off)):
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]), (graph, i, k)
        for k in p_on:
            assert torch.equal(p_on[k], p_off[k]), (graph, k)
