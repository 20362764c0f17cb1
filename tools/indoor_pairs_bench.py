#!/usr/bin/env python
"""Indoor descriptor pair builder (csrc/indoor_pairs.hip) at the reference's shape (P = 2, N = 5000,
n_sub = 2500, M = 512): ONE JSON line, also written to profiles/f26_indoor_pairs_bench.json.

    python tools/indoor_pairs_bench.py

builder_ms            HIP events around one build (P pairs), median of --runs, alternating in --rounds blocks with
desc_builder_ms       the outdoor descriptor builder (usip_amd.desc_pairs) at equal (P, N, M, n_sub) in the same process
fps_ms / fps_share    usip_fps_f32 alone on the same candidates: 2P clouds, M - 1 dependent rounds, one workgroup each
twin_ms_per_call      the host twin (usip_indoor_pairs_build_f32_cpu) on --threads threads, one call of P pairs
step_ms               one training step (frozen detector forward + IndoorDescriptorStep, graph replay, Adam): on a pre-built
                      batch, with the builder before each step on the same stream, and prefetched on a side stream; the
                      legs alternate --rounds times, medians reported
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f26_indoor_pairs_bench.json"))
    args = ap.parse_args()
    import torch
    from usip_amd import desc_pairs, indoor_pairs, ops, synth
    from usip_amd.networks import IndoorOptions, build_detector
    P, N, M = args.pairs, args.n, args.m
    opt = IndoorOptions(input_pc_num=N, node_num=M, batch_size=P, sigma_max=5.0)     # a seeded detector's sigmas are large
    recipe = indoor_pairs.IndoorPairRecipe.scenenn(opt)
    root = tempfile.mkdtemp(prefix="scenenn_bench_")
    indoor_pairs.synthetic_scenenn(root, frames=args.frames, rows=args.rows, seed=0, modes=("train",))
    frames, pairs, icp = indoor_pairs.load_root(root, "train")
    S = len(pairs)
    line = dict(metric="indoor_pair_builder", pairs=P, n=N, m=M, cs=recipe.Cs, n_sub=recipe.n_sub, frame_rows=args.rows,
                samples=S)
    ids_h = [np.random.default_rng(e).permutation(S)[:P] for e in range(8)]
    indoor_pairs.build_cpu(recipe, frames, pairs, icp, ids_h[0], P, seed=1, step=0, num_threads=args.threads)
    t = []
    for i in range(5):
        t0 = time.perf_counter()
        indoor_pairs.build_cpu(recipe, frames, pairs, icp, ids_h[i], P, seed=1, step=i, num_threads=args.threads)
        t.append(time.perf_counter() - t0)
    line["twin_threads"], line["twin_ms_per_call"] = args.threads, round(1e3 * float(np.median(t)), 2)

    dev = torch.device("cuda:0")
    bank = indoor_pairs.IndoorPairBank.from_arrays(frames, pairs, icp, dev)
    builder = indoor_pairs.IndoorPairBuilder(bank, recipe, P, dev, seed=1)
    eight = [np.concatenate([f, f[:, :1]], 1) for f in frames]
    poses = np.stack([np.eye(4)] * len(eight))
    dbank = desc_pairs.PosedScanBank(eight, poses, [0] * len(eight), dev, min_points=N)
    drecipe = desc_pairs.DescriptorPairRecipe(N=N, M=M, Cs=recipe.Cs, n_sub=recipe.n_sub)
    dbuilder = desc_pairs.DescriptorPairBuilder(dbank, drecipe, P, dev, seed=1)
    ids = [torch.tensor(i, dtype=torch.int32, device=dev) for i in ids_h]
    dids = [torch.tensor(i % len(eight), dtype=torch.int32, device=dev) for i in ids_h]
    buf, dbuf = indoor_pairs.empty_batch(builder.c, P, dev), desc_pairs.empty_batch(dbuilder.c, P, dev)

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

    new, old = [], []
    for _ in range(args.rounds):                             # alternating blocks in the same process
        old.append(timed(lambda i: dbuilder.build(dids[i % 8], i, out=dbuf), args.runs))
        new.append(timed(lambda i: builder.build(ids[i % 8], i, out=buf), args.runs))
    line["builder_ms"], line["builder_ms_all"] = round(float(np.median(new)), 4), [round(x, 4) for x in new]
    line["desc_builder_ms"], line["desc_builder_ms_all"] = round(float(np.median(old)), 4), [round(x, 4) for x in old]
    line["builder_over_desc_builder"] = round(line["builder_ms"] / line["desc_builder_ms"], 4)
    cand, first = builder.workspace_candidates()
    line["fps_ms"] = round(timed(lambda i: ops.fps(cand, first, M), args.runs), 4)
    line["fps_share"] = round(line["fps_ms"] / line["builder_ms"], 3)

    ops.set_matmul_mode("f32x2")
    det = build_detector("ball", opt)
    sd = det.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    state = {k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in filled.items()}
    tr = indoor_pairs.IndoorDescriptorTrainer(builder, "ball", state, opt, dev, seed=0, graph=True)
    for i in range(3):
        tr.train_step(builder.build(ids[i], i), epoch=0)
    builder.build(ids[0], 0, out=buf)
    step_no = [100]

    def leg_prebuilt():
        for _ in range(args.steps):
            tr.train_step(buf, epoch=0)

    def leg_sequential():
        for _ in range(args.steps):
            step_no[0] += 1
            tr.train_step(builder.build(ids[step_no[0] % 8], step_no[0], out=buf), epoch=0)

    def leg_prefetched():
        sched = []
        for _ in range(args.steps):
            step_no[0] += 1
            sched.append((ids[step_no[0] % 8], step_no[0]))
        for b in builder.prefetch(sched):
            tr.train_step(b, epoch=0)

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
    for k, v in res.items():
        line["step_ms_" + k] = round(float(np.median(v)), 4)
        line["step_ms_%s_all" % k] = [round(x, 4) for x in v]
    line["build_hidden_by_prefetch"] = round(
        1.0 - (line["step_ms_prefetched"] - line["step_ms_prebuilt"]) /
        max(line["step_ms_sequential"] - line["step_ms_prebuilt"], 1e-9), 3)
    line["last_loss"] = float(tr.last_loss)
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
