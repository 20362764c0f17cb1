#!/usr/bin/env python
"""Describing a scene's fragments from two networks (usip_amd.fragment_batch) at the reference's evaluation
shape -- a 57-fragment scene (Redwood livingroom1's count) of 100 000-row fragments, N = 10240, n_sub = 5120, M = 512, top 512,
batches of 8: ONE JSON line, also written to profiles/f27_fragment_describe_bench.json.

    python tools/fragment_describe_bench.py

builder_ms            HIP events around one build of a batch (csrc/fragment_batch.hip), median over --runs
fps_ms / fps_share    usip_fps_f32 alone on the same candidates
detector_ms, selection_ms, descriptor_ms
                      the eval-mode Ball detector, select_keypoints_device and the eval-mode DescriptorLiteOldGlobal on one
                      batch, each between its own events, medians over --runs
describe_ms           FragmentDescriber.describe on one batch; scene_ms: the 57 fragments in 8 batches, wall clock, synchronised
                      once at the end
twin_ms_per_batch     the host twin (usip_fragment_batch_build_f32_cpu) on --threads threads, one batch
parent_ms_per_fragment
                      what the parent commit offers, in the same process: a numpy restatement of the reference's loader
                      (two choices and a float64 FPS of 512 rounds over 5120 candidates) per fragment on the host, the upload,
                      FragmentEvaluator.add_fragment; over --parent-fragments fragments.  parent_loader_ms is its host part.
The networks are seeded, not trained: the figures are of the launches, not of a model's quality."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_loader(frame, N, n_sub, M, rng):
    """RedwoodLoader.__getitem__ restated: (pc [3,N], sn [4,N], node [3,M]) float32."""
    rows = frame[rng.choice(frame.shape[0], N, replace=False)]
    pts = rows[rng.choice(N, n_sub, replace=False), :3]
    far = np.zeros((M, 3))
    far[0] = pts[rng.integers(len(pts))]
    dist = ((far[0] - pts) ** 2).sum(axis=1)
    for i in range(1, M):
        far[i] = pts[np.argmax(dist)]
        dist = np.minimum(dist, ((far[i] - pts) ** 2).sum(axis=1))
    return rows[:, :3].T.astype(np.float32), rows[:, 3:7].T.astype(np.float32), far.T.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=57)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--n", type=int, default=10240)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--top", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-fragments", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f27_fragment_describe_bench.json"))
    args = ap.parse_args()
    import torch
    from usip_amd import fragment_batch as fb, fragments as fr, inference, ops, synth
    from usip_amd.evaluation import select_keypoints_device
    from usip_amd.networks import DescriptorLiteOldGlobal, IndoorDetectorOptions, IndoorOptions, build_detector
    F, N, M, B = args.fragments, args.n, args.m, args.batch
    rng = np.random.default_rng(27)
    frames = [np.concatenate([synth.make_cloud(rng, args.rows, "slab:3").T, synth.make_normals(rng, args.rows, 4).T],
                             1).astype(np.float32) for _ in range(F)]
    det_opt = IndoorDetectorOptions(input_pc_num=N, node_num=M)
    recipe = fb.FragmentBatchRecipe.match3d(det_opt)
    line = dict(metric="fragment_describe", fragments=F, rows=args.rows, n=N, n_sub=recipe.n_sub, m=M, top=args.top, batch=B)

    ids0 = list(range(B))
    fb.build_cpu(recipe, frames, ids0, seed=1, num_threads=args.threads)
    t = []
    for i in range(3):
        t0 = time.perf_counter()
        fb.build_cpu(recipe, frames, ids0, seed=1, step=i, num_threads=args.threads)
        t.append(time.perf_counter() - t0)
    line["twin_threads"], line["twin_ms_per_batch"] = args.threads, round(1e3 * float(np.median(t)), 2)

    dev = torch.device("cuda:0")
    bank = fb.FragmentScanBank.from_arrays(frames, dev)
    builder = fb.FragmentBatchBuilder(bank, recipe, seed=1)
    det = build_detector("ball", det_opt)
    sd = det.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    det.load_state_dict({k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in filled.items()})
    det = det.to(dev).eval()
    torch.manual_seed(0)
    desc = DescriptorLiteOldGlobal(IndoorOptions(input_pc_num=N, node_num=M)).to(dev).eval()
    describer = fb.FragmentDescriber(det, desc, builder, nms_radius=0.1, top=args.top)
    ids = torch.arange(B, dtype=torch.int32, device=dev)

    def timed(fn, runs):
        for i in range(3):
            fn(i)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
        for i, (s, e) in enumerate(ev):
            s.record()
            fn(i)
            e.record()
        torch.cuda.synchronize()
        return round(float(np.median([s.elapsed_time(e) for s, e in ev])), 4)

    line["builder_ms"] = timed(lambda i: builder.build(ids, i), args.runs)
    ws = builder._workspace(B)
    o_c, o_f = (ops.fragment_batch_workspace_offset(builder.c, B, p) for p in (1, 2))
    cand = ws[o_c:o_c + B * 3 * recipe.n_sub * 4].view(torch.float32).view(B, 3, recipe.n_sub)
    first = ws[o_f:o_f + B * 4].view(torch.int32)
    line["fps_ms"] = timed(lambda i: ops.fps(cand, first, M), args.runs)
    line["fps_share"] = round(line["fps_ms"] / line["builder_ms"], 3)
    batch = builder.build(ids, 0)
    keypoints, sigmas = inference.run_model(det, batch["pc"], batch["sn"], batch["node"])
    kp, count = select_keypoints_device(keypoints, sigmas, 0.1, args.top)
    line["detector_ms"] = timed(lambda i: inference.run_model(det, batch["pc"], batch["sn"], batch["node"]), args.runs)
    line["selection_ms"] = timed(lambda i: select_keypoints_device(keypoints, sigmas, 0.1, args.top), args.runs)
    line["descriptor_ms"] = timed(lambda i: describer._describe(batch["pc"], batch["sn"], kp), args.runs)
    line["describe_ms"] = timed(lambda i: describer.describe(ids, i), args.runs)
    scene = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for base in range(0, F, B):
            describer.describe(list(range(base, min(base + B, F))))
        torch.cuda.synchronize()
        scene.append(1e3 * (time.perf_counter() - t0))
    line["scene_ms"], line["scene_ms_all"] = round(float(np.median(scene)), 2), [round(x, 2) for x in scene]
    line["scene_ms_per_fragment"] = round(line["scene_ms"] / F, 3)

    ev = fr.FragmentEvaluator(det, desc, None, dev, nms_radius=0.1, top=args.top)
    prng = np.random.default_rng(1)
    host, total = [], []
    for rep in range(2):                                      # the first pass warms the B = 1 launches up
        host, total = [], []
        for i in range(min(args.parent_fragments, F)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pc, sn, node = numpy_loader(frames[i], N, recipe.n_sub, M, prng)
            t1 = time.perf_counter()
            up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).unsqueeze(0) for a in (pc, sn, node)]
            ev.add_fragment(i, up[0], up[1], up[2], bank.xyz(i))
            torch.cuda.synchronize()
            host.append(1e3 * (t1 - t0))
            total.append(1e3 * (time.perf_counter() - t0))
    line["parent_fragments"] = len(total)
    line["parent_loader_ms"] = round(float(np.median(host)), 2)
    line["parent_ms_per_fragment"] = round(float(np.median(total)), 2)
    line["parent_over_this"] = round(line["parent_ms_per_fragment"] / line["scene_ms_per_fragment"], 2)
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
