#!/usr/bin/env python
"""Descriptor pair builder (csrc/desc_pairs.hip) at the reference's default shape: one JSON line.

    python tools/desc_pairs_bench.py                         # builder, yardstick, FPS share, step legs, host twin cost
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/desc_pairs_bench.py --quick
    python tools/desc_pairs_bench.py --kernel-stats DIR      # + the kernels' us from that trace

builder_ms            HIP events around one build (P pairs), median of --runs, alternating in --rounds blocks with
detector_builder_ms   the detector builder (usip_amd.pairs, tools/pair_builder_bench.py's own measurement) at equal
                      (P, N, M, n_sub) on the same bank: the yardstick, since the per-slot and FPS work per cloud are its own
fps_ms                usip_fps_f32 alone on the same candidates (its share of the builder)
points_us             cloud_points_kernel<..., CloudView> from a rocprofv3 --stats run (average), with algorithmic bytes and
                      the fraction of 8 TB/s those bytes would take; select_mine_us: desc_select_kernel + desc_mine_kernel
detector_forward_ms   the frozen detector's eval-mode forward on cat(anchor, positive)
descriptor_step_ms    DescriptorStep alone (graph replay, Adam) on a static batch
step_ms               one training step = frozen-detector forward + DescriptorStep: on a pre-built batch, with the builder
                      run before each step on the same stream, and prefetched (built on a side stream while the previous
                      step runs); the three legs alternate --rounds times in one process, medians reported
twin_ms_per_pair      the host twin (usip_desc_pairs_build_f32_cpu) on one core, and the pairs/s --procs processes make
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

_CPU = {}


def _twin_work(i):
    from usip_amd import desc_pairs
    a = _CPU
    ids = np.random.default_rng(i).permutation(len(a["scans"]))[:a["P"]]
    desc_pairs.build_cpu(a["recipe"], a["scans"], a["poses"], a["seq"], ids, a["P"], seed=1, step=i)


def twin_cost(recipe, scans, poses, seq, P, procs, calls):
    """One call of P pairs on one core, then `calls` calls on `procs` forked worker processes (the reference's DataLoader
    uses worker processes).  Runs before the GPU is touched, so no worker ever opens it."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    _CPU.update(recipe=recipe, scans=scans, poses=poses, seq=seq, P=P)
    _twin_work(0)
    t0 = time.perf_counter()
    _twin_work(1)
    one = (time.perf_counter() - t0) / P
    with ProcessPoolExecutor(procs, mp_context=multiprocessing.get_context("fork")) as ex:
        list(ex.map(_twin_work, range(procs)))                   # start the workers
        t0 = time.perf_counter()
        list(ex.map(_twin_work, range(procs, procs + calls)))
        wall = time.perf_counter() - t0
    return dict(twin_ms_per_pair_1core=round(1e3 * one, 2), twin_processes=procs,
                twin_pairs_per_s=round(calls * P / wall, 1))


def kernels_from_stats(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                if "cloud_" in name and "CloudView" not in name:         # the detector builder's instantiation
                    continue
                for k in ("cloud_points_kernel", "desc_select_kernel", "desc_mine_kernel", "cloud_nodes_kernel"):
                    if k in name:
                        out[k] = float(row["AverageNs"]) / 1e3
    if "cloud_points_kernel" not in out:
        raise RuntimeError("no cloud_points_kernel<..., CloudView> row in %s" % path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--cs", type=int, default=4)
    ap.add_argument("--rows", type=int, default=20480)
    ap.add_argument("--scans", type=int, default=40, help="scans per sequence (two sequences)")
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--twin-calls", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="builds only (for a rocprofv3 trace)")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    from usip_amd import desc_pairs, synth
    from usip_amd.networks import DetectorOptions
    P, N, M, Cs = args.pairs, args.n, args.m, args.cs
    opt = DetectorOptions(surface_normal_len=Cs, node_knn_k_1=16, input_pc_num=N, node_num=M)
    recipe = desc_pairs.DescriptorPairRecipe.kitti(opt)
    seqs = desc_pairs.synthetic_sequences(2, args.scans, args.rows, 0.8, seed=0)
    scans = [s for q in seqs for s in seqs[q][0]]
    poses = np.concatenate([seqs[q][1] for q in seqs])
    seq = [q for q in seqs for _ in seqs[q][0]]
    S = len(scans)
    line = dict(metric="desc_pair_builder", pairs=P, n=N, m=M, cs=Cs, n_sub=recipe.n_sub, scan_rows=args.rows, scans=S)
    if not args.quick:
        line.update(twin_cost(recipe, scans, poses, seq, P, args.procs, args.twin_calls))    # before the GPU is touched

    import torch
    from usip_amd import inference, ops, pairs
    from usip_amd.networks import build_detector
    dev = torch.device("cuda:0")
    bank = desc_pairs.PosedScanBank(scans, poses, seq, dev, min_points=N)
    builder = desc_pairs.DescriptorPairBuilder(bank, recipe, P, dev, seed=1)
    yard_recipe = pairs.PairRecipe(N=N, M=M, Cs=Cs, n_sub=recipe.n_sub)
    yard = pairs.PairBuilder(bank, yard_recipe, P, dev, seed=1)
    ids = [torch.tensor(pairs.epoch_order(S, 1, e)[:P], device=dev) for e in range(8)]
    buf, ybuf = desc_pairs.empty_batch(builder.c, P, dev), pairs.empty_batch(yard_recipe, P, dev)

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

    if args.quick:
        line["builder_ms"] = round(timed(lambda i: builder.build(ids[i % 8], i, out=buf), args.runs), 4)
        print(json.dumps(line), flush=True)
        return
    new, old = [], []
    for _ in range(args.rounds):                             # alternating blocks on the same box
        old.append(timed(lambda i: yard.build(ids[i % 8], i, out=ybuf), args.runs))
        new.append(timed(lambda i: builder.build(ids[i % 8], i, out=buf), args.runs))
    line["builder_ms"], line["builder_ms_all"] = round(float(np.median(new)), 4), [round(x, 4) for x in new]
    line["detector_builder_ms"] = round(float(np.median(old)), 4)
    line["detector_builder_ms_all"] = [round(x, 4) for x in old]
    line["builder_over_detector_builder"] = round(line["builder_ms"] / line["detector_builder_ms"], 4)
    cand, first = builder.workspace_candidates()
    line["fps_ms"] = round(timed(lambda i: ops.fps(cand, first, M), args.runs), 4)
    line["fps_share"] = round(line["fps_ms"] / line["builder_ms"], 3)
    nbytes = 2 * P * (N * (32 + 4 * (3 + Cs)) + recipe.n_sub * (32 + 12))
    line["points_bytes"] = nbytes
    if args.kernel_stats:
        k = kernels_from_stats(args.kernel_stats)
        line["points_us"] = round(k["cloud_points_kernel"], 2)
        line["points_frac_8TBps"] = round(nbytes / 8e12 / (k["cloud_points_kernel"] * 1e-6), 3)
        line["select_mine_us"] = round(k.get("desc_select_kernel", 0.0) + k.get("desc_mine_kernel", 0.0), 2)
        line["nodes_us"] = round(k.get("cloud_nodes_kernel", 0.0), 2)
    else:
        line["points_us"] = line["select_mine_us"] = "not measured (no --kernel-stats)"
    torch.cuda.synchronize()
    line["neg_fail"] = int(buf["neg_fail"])

    ops.set_matmul_mode("f32x2")
    det = build_detector("ball", opt)
    sd = det.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    state = {k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in filled.items()}
    tr = desc_pairs.DescriptorTrainer(builder, "ball", state, opt, dev, seed=0, graph=True)
    for i in range(3):
        tr.train_step(builder.build(ids[i], i))
    builder.build(ids[0], 0, out=buf)
    cat = [torch.cat((buf["anc_" + k], buf["pos_" + k]), 0) for k in ("pc", "sn", "node")]
    line["detector_forward_ms"] = round(timed(lambda i: inference.run_model(tr.detector, *cat), args.runs), 4)
    static = tr.descriptor_batch(buf)
    static = tr.st.static_batch(static) or static
    line["descriptor_step_ms"] = round(timed(lambda i: tr.st.step(static), args.runs), 4)
    line["detector_forward_over_descriptor_step"] = round(line["detector_forward_ms"] / line["descriptor_step_ms"], 4)
    step_no = [100]

    def leg_prebuilt():
        for _ in range(args.steps):
            tr.train_step(buf)

    def leg_sequential():
        for _ in range(args.steps):
            step_no[0] += 1
            tr.train_step(builder.build(ids[step_no[0] % 8], step_no[0], out=buf))

    def leg_prefetched():
        sched = []
        for _ in range(args.steps):
            step_no[0] += 1
            sched.append((ids[step_no[0] % 8], step_no[0]))
        for b in builder.prefetch(sched):
            tr.train_step(b)

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
    loss = float(tr.last_loss.detach())
    assert math.isfinite(loss)
    for k, v in res.items():
        line["step_ms_" + k] = round(float(np.median(v)), 4)
        line["step_ms_%s_all" % k] = [round(x, 4) for x in v]
    line["prefetched_over_prebuilt"] = round(line["step_ms_prefetched"] / line["step_ms_prebuilt"], 4)
    line["gpu_pairs_per_s_builder"] = round(1e3 * P / line["builder_ms"], 1)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
