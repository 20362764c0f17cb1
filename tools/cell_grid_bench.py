"""Stand-alone times of the two brute-force searches of the detector step and of the cell-grid route that replaces them
(csrc/cell_grid.hip), at the bench's sizes: B = 16 clouds, N = 16384 points, M = 512 nodes / keypoints, radius 2, K = 64.

    python tools/cell_grid_bench.py [slab cube slab:8 ...]

HIP events around 20 back-to-back launches after a warm-up; the mean per launch and the share of rows the grid answered.
"""
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from usip_amd import ops, synth  # noqa: E402

DEV = "cuda:0"
B, N, M, K, R = 16, 16384, 512, 64, 2.0


def timeit(fn, reps=20):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    for kind in (sys.argv[1:] or ["slab", "cube", "slab:8"]):
        rng = np.random.default_rng(3)
        x = np.stack([synth.make_cloud(rng, N, kind) for _ in range(B)])
        node = np.ascontiguousarray(np.stack([x[b][:, rng.permutation(N)[:M]] for b in range(B)]))
        kp = (node + rng.normal(0, 0.5, node.shape)).astype(np.float32)            # keypoints: near the cloud, not on it
        tx, tn, tk = (torch.from_numpy(a).to(DEV) for a in (x, node, kp))
        grid = ops.cell_grid_build(tx, R * ops.cell_edge_factor(), ops.ball_block_limit(N, K))
        idx, r_bq = ops.ball_query_grid(tn, grid, R, K, with_route=True)
        d, j, r_nn = ops.nearest_grid(tk, grid, with_route=True)
        assert torch.equal(idx, ops.ball_query_coords(tn, tx, R, K))
        wd, wj = ops.nearest(tk, tx)
        assert torch.equal(j, wj) and torch.equal(d.view(torch.int32), wd.view(torch.int32))
        t = dict(bq_scan=timeit(lambda: ops.ball_query_coords(tn, tx, R, K)), nn_scan=timeit(lambda: ops.nearest(tk, tx)),
                 build=timeit(lambda: ops.cell_grid_build(tx, R * ops.cell_edge_factor(), ops.ball_block_limit(N, K))),
                 bq_grid=timeit(lambda: ops.ball_query_grid(tn, grid, R, K)), nn_grid=timeit(lambda: ops.nearest_grid(tk, grid)))
        h = grid.header()[0]
        print("%-7s ball_query_coords %6.1f us  nearest %6.1f us  sum %6.1f | cell_grid_build %5.1f  ball_query_grid %5.1f "
              "(%.0f%% grid)  nearest_grid %5.1f (%.0f%% grid)  sum %6.1f | dim %s edge %.3f"
              % (kind, t["bq_scan"], t["nn_scan"], t["bq_scan"] + t["nn_scan"], t["build"], t["bq_grid"],
                 100 * float(r_bq.float().mean()), t["nn_grid"], 100 * float(r_nn.float().mean()),
                 t["build"] + t["bq_grid"] + t["nn_grid"], h["dim"], h["edge"]), flush=True)


if __name__ == "__main__":
    main()
