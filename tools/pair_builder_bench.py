#!/usr/bin/env python
"""Training-pair builder (csrc/pairs.hip) at the KITTI shape: one JSON line.

    python tools/pair_builder_bench.py                       # builder, FPS share, step legs, CPU recipe cost
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pair_builder_bench.py --quick
    python tools/pair_builder_bench.py --kernel-stats DIR    # + cloud_points_kernel us from that trace

builder_ms      HIP events around one build (P pairs), median of --runs
fps_ms          usip_fps_f32 alone on the same candidates, median of --runs (its share of the builder)
points_us       cloud_points_kernel<..., PairView> from a rocprofv3 --stats run (average), with algorithmic bytes and the
                fraction of 8 TB/s those bytes would take
step_ms         DetectorStep (graph replay, Adam) per step: on a pre-built batch, with the builder run before each step on
                the same stream, and prefetched (built on a side stream while the previous step replays); the three legs
                alternate --rounds times in one process, medians reported
cpu_ms_per_pair a numpy restatement of the reference's KITTI recipe (subsample, float64 FPS over N/3, augment, transform)
                on one core, and the pairs/s --procs worker processes make (the DataLoader's form: no shared GIL)
"""
import argparse
import csv
import glob
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def numpy_pair(scan, rng, N, M, Cs):
    """The reference's per-pair work (KittiLoader.__getitem__ + augment + transform_pc_pytorch), restated in numpy."""
    def instance():
        pc = scan[rng.choice(scan.shape[0], N, replace=False)]
        sn, pc = pc[:, 3:3 + Cs].copy(), pc[:, 0:3]
        sub = pc[rng.choice(N, int(N / 3), replace=False)].astype(np.float64)
        nodes = np.zeros((M, 3))
        nodes[0] = sub[rng.integers(len(sub))]
        d = ((nodes[0] - sub) ** 2).sum(1)
        for i in range(1, M):
            nodes[i] = sub[np.argmax(d)]
            d = np.minimum(d, ((nodes[i] - sub) ** 2).sum(1))
        return pc, sn, nodes
    out = [instance(), instance()]
    a = rng.uniform() * 2 * np.pi
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    jp, js, jn = (np.clip(s * rng.standard_normal(sh), -c, c) for s, c, sh in
                  ((0.04, 0.12, (2, N, 3)), (0.01, 0.05, (2, N, Cs)), (0.04, 0.12, (2, M, 3))))
    scale = rng.uniform(0.9, 1.1)
    res = []
    for b, (pc, sn, nodes) in enumerate(out):
        pc = (pc @ R + jp[b]) * scale
        sn[:, 0:3] = sn[:, 0:3] @ R
        sn += js[b]
        nodes = (nodes @ R + jn[b]) * scale
        res.append((pc.T.astype(np.float32), sn.T.astype(np.float32), nodes.T.astype(np.float32)))
    Rd = R.astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, (3, 1)).astype(np.float32)
    pc, sn, nodes = res[1]
    return res[0], (Rd @ pc + shift, sn, Rd @ nodes + shift)


_CPU = {}


def _cpu_work(i):
    a = _CPU
    numpy_pair(a["scans"][i % len(a["scans"])], np.random.default_rng(i), a["N"], a["M"], a["Cs"])


def cpu_cost(scans, N, M, Cs, procs, pairs):
    """One pair on one core, then `pairs` pairs on `procs` forked worker processes (the reference's DataLoader uses
    worker processes: no GIL between them).  Runs before torch is imported, so no worker ever touches the GPU."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    _CPU.update(scans=scans, N=N, M=M, Cs=Cs)
    _cpu_work(0)
    t0 = time.perf_counter()
    _cpu_work(1)
    one = time.perf_counter() - t0
    with ProcessPoolExecutor(procs, mp_context=multiprocessing.get_context("fork")) as ex:
        list(ex.map(_cpu_work, range(procs)))                    # start the workers
        t0 = time.perf_counter()
        list(ex.map(_cpu_work, range(procs, procs + pairs)))
        wall = time.perf_counter() - t0
    return dict(cpu_ms_per_pair_1core=round(1e3 * one, 2), cpu_processes=procs,
                cpu_pairs_per_s=round(pairs / wall, 1))


def points_from_stats(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True) if os.path.isdir(path) else [path]
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                if "cloud_points_kernel" in name and "PairView" in name:
                    return float(row["AverageNs"]) / 1e3, f
    raise RuntimeError("no cloud_points_kernel<..., PairView> row in %s" % path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--cs", type=int, default=4)
    ap.add_argument("--rows", type=int, default=20480)
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--runs", type=int, default=60)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--cpu-pairs", type=int, default=64)
    ap.add_argument("--quick", action="store_true", help="builds only (for a rocprofv3 trace)")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    from usip_amd import synth
    P, N, M, Cs = args.pairs, args.n, args.m, args.cs
    rng = np.random.default_rng(0)
    scans = [np.concatenate([synth.make_cloud(rng, args.rows, "slab").T, synth.make_normals(rng, args.rows, 5).T], 1)
             .astype(np.float32) for _ in range(args.scans)]
    line = dict(metric="pair_builder", pairs=P, n=N, m=M, cs=Cs, scan_rows=args.rows)
    if not args.quick:
        line.update(cpu_cost(scans, N, M, Cs, args.procs, args.cpu_pairs))    # before the GPU is touched

    import torch
    from usip_amd import ops, pairs
    from usip_amd.networks import DetectorOptions
    from usip_amd.step import DetectorStep
    dev = torch.device("cuda:0")
    opt = DetectorOptions(surface_normal_len=Cs, node_knn_k_1=16, input_pc_num=N, node_num=M)
    recipe = pairs.PairRecipe.kitti(opt)
    builder = pairs.PairBuilder(pairs.ScanBank(scans, dev), recipe, P, dev, seed=1)
    ids = [torch.tensor(pairs.epoch_order(args.scans, 1, e)[:P], device=dev) for e in range(8)]
    buf = pairs.empty_batch(recipe, P, dev)

    def timed(fn, runs):
        for i in range(3):
            fn(i)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
        for i, (s, e) in enumerate(ev):
            s.record()
            fn(i)
            e.record()
        torch.cuda.synchronize()
        return float(np.median([s.elapsed_time(e) for s, e in ev]))

    line["builder_ms"] = round(timed(lambda i: builder.build(ids[i % 8], i, out=buf), args.runs), 4)
    if args.quick:
        print(json.dumps(line), flush=True)
        return
    cand, first = builder.workspace_candidates()
    line["fps_ms"] = round(timed(lambda i: ops.fps(cand, first, M), args.runs), 4)
    line["fps_share"] = round(line["fps_ms"] / line["builder_ms"], 3)
    nbytes = 2 * P * (N * (32 + 4 * (3 + Cs)) + recipe.n_sub * (32 + 12))
    line["points_bytes"] = nbytes
    if args.kernel_stats:
        us, _ = points_from_stats(args.kernel_stats)
        line["points_us"] = round(us, 2)
        line["points_frac_8TBps"] = round(nbytes / 8e12 / (us * 1e-6), 3)
    else:
        line["points_us"] = "not measured (no --kernel-stats)"

    ops.set_matmul_mode("f32x2")
    torch.manual_seed(0)
    st = DetectorStep("ball", opt, dev, with_optimizer=True, graph=True)
    for i in range(3):
        st.step(builder.build(ids[i], i))
    static = st.static_batch(buf)
    builder.build(ids[0], 0, out=static)
    step_no = [100]

    def leg_prebuilt():
        for _ in range(args.steps):
            st.step(static)

    def leg_sequential():
        for _ in range(args.steps):
            step_no[0] += 1
            builder.build(ids[step_no[0] % 8], step_no[0], out=static)
            st.step(static)

    def leg_prefetched():
        sched = []
        for _ in range(args.steps):
            step_no[0] += 1
            sched.append((ids[step_no[0] % 8], step_no[0]))
        for b in builder.prefetch(sched):
            st.step(b)

    legs = dict(prebuilt=leg_prebuilt, sequential=leg_sequential, prefetched=leg_prefetched)
    res = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            res[k].append(s.elapsed_time(e) / args.steps)
    loss = float(st.last["loss"].detach())
    assert math.isfinite(loss)
    for k, v in res.items():
        line["step_ms_" + k] = round(float(np.median(v)), 4)
        line["step_ms_%s_all" % k] = [round(x, 4) for x in v]
    line["prefetched_over_prebuilt"] = round(line["step_ms_prefetched"] / line["step_ms_prebuilt"], 4)
    line["gpu_pairs_per_s_builder"] = round(1e3 * P / line["builder_ms"], 1)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
