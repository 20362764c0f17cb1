#!/usr/bin/env python
"""Times of the f-7 scan preparation (usip_amd/prepare.py) on the 119 768-point ring scan of tests/prepare_oracle.py:
per-stage device time -- (a) the sort along x, (b) the neighbour kernel, (c) normals, (d) cell keys, (e) sort + segment starts,
(f) the cell average -- next to the library's host twin on `--threads` threads and the independent oracle (scipy cKDTree +
numpy.linalg.eigh + a numpy grid, tests/prepare_oracle.py), and the share of the n^2 pairs the pruned neighbour walk visits
(from the tile counts the kernel writes).  One JSON line.

    python tools/prepare_bench.py [--reps 10] [--threads 16] [--skip-host]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows; the whole
pipeline (one call of ScanPreparer, its one host synchronisation included) is timed on the wall clock, median of 5."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import prepare_oracle as po                     # noqa: E402
from usip_amd import ops, prepare               # noqa: E402


def device_us(fn, reps, windows=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / reps)
    return float(np.median(out)), [round(v, 1) for v in out]


def wall_ms(fn, reps=5, warmup=1):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--leaf", type=float, default=0.2)
    ap.add_argument("--skip-host", action="store_true", help="leave the all-pairs host twin out (seconds per call)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prepare_bench needs a GPU"
    K = args.k
    scan = po.ring_scan(3)
    n = len(scan)
    prep = prepare.ScanPreparer("cuda:0", k=K, leaf=args.leaf)
    pts = torch.from_numpy(scan).cuda()
    res = {"metric": "f7_prepare", "device": torch.cuda.get_device_name(0), "host": platform.node(), "points": n, "k": K,
           "leaf": args.leaf}

    sort_x = lambda: torch.sort(pts[:, 0], stable=True).indices.to(torch.int32)     # noqa: E731
    perm = sort_x()
    idx, visits = ops.scan_knn(pts, perm, K, want_visits=True)
    tiles = (n + 255) // 256
    res["tiles_visited_share"] = float(visits.double().sum()) / tiles / tiles       # = the share of the n^2 pairs walked
    res["tiles_visited_max_of_%d" % tiles] = int(visits.max())
    nrm64, _ = ops.scan_normals(pts, idx)
    lo, hi = torch.aminmax(pts[:, :3], dim=0)
    lohi = torch.cat((lo, hi)).contiguous()
    keys = ops.scan_voxel_keys(pts, lohi, args.leaf)

    def segments():
        skeys, order = torch.sort(keys, stable=True)
        cells, counts = torch.unique_consecutive(skeys, return_counts=True)
        start = torch.zeros(cells.shape[0] + 1, dtype=torch.int32, device=pts.device)
        start[1:] = torch.cumsum(counts, 0)
        return order.to(torch.int32), start

    order, start = segments()
    res["rows_out"] = int(start.shape[0]) - 1
    stages = {"sort_x_us": sort_x, "knn_us": lambda: ops.scan_knn(pts, perm, K),
              "normals_us": lambda: ops.scan_normals(pts, idx), "voxel_keys_us": lambda: ops.scan_voxel_keys(pts, lohi, args.leaf),
              "sort_keys_segments_us": segments, "voxel_average_us": lambda: ops.scan_voxel_average(pts, nrm64, order, start)}
    for name, fn in stages.items():
        res[name], res[name + "_all"] = device_us(fn, args.reps)
    res["device_stages_total_ms"] = sum(res[k] for k in stages) * 1e-3
    res["device_pipeline_wall_ms"] = wall_ms(lambda: (prep(pts), torch.cuda.synchronize()))
    res["distances_per_s"] = res["tiles_visited_share"] * float(n) * n / (res["knn_us"] * 1e-6)

    # the independent oracle on the host: cKDTree(workers) + eigh + numpy grid
    def oracle():
        want, _ = po.neighbours(scan, K, workers=args.threads)
        o = po.normals(scan, want)
        po.grid(scan, np.concatenate((o["normal"], o["curvature"][:, None]), 1), args.leaf)

    t0 = time.perf_counter()
    want, _ = po.neighbours(scan, K, workers=args.threads)
    res["oracle_knn_ms"] = (time.perf_counter() - t0) * 1e3
    res["oracle_threads"] = args.threads
    res["oracle_pipeline_ms"] = wall_ms(oracle, reps=3, warmup=0)
    res["device_over_oracle"] = res["device_pipeline_wall_ms"] / res["oracle_pipeline_ms"]
    res["knn_equals_oracle"] = bool(np.array_equal(idx.cpu().numpy(), want))
    if not args.skip_host:
        res["host_threads"] = args.threads
        t0 = time.perf_counter()
        hidx = prepare.knn_cpu(scan, K, args.threads)
        res["host_knn_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["knn_equals_host"] = bool(np.array_equal(idx.cpu().numpy(), hidx))
        res["host_normals_ms"] = wall_ms(lambda: prepare.normals_cpu(scan, hidx, K), reps=3, warmup=0)
        h64 = prepare.normals_cpu(scan, hidx, K)[0]
        res["host_grid_ms"] = wall_ms(lambda: prepare.grid_cpu(scan, h64, args.leaf), reps=3, warmup=0)
        res["host_total_ms"] = res["host_knn_all_pairs_ms"] + res["host_normals_ms"] + res["host_grid_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
