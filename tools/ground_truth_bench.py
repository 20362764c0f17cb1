#!/usr/bin/env python
"""Times of a fragment scene's ground truth (usip_amd/ground_truth.py) on one synthetic scene of 57 fragments,
all 1596 pairs, `--points` points per fragment, grid-averaged at `--leaf` (0.01 m, the reference's).  Per stage, HIP events
summed over the scene's batches, the median of `--repeats` passes after a warm-up batch: the moved-x keys and their sort, the
reach kernel, the selection (the key sort) and the information sum.  Beside it, in the same process:
  (a) the library's host twin (csrc/ground_truth_cpu.cpp, prune on) on `--threads` threads, timed on `--host-pairs` evenly
      spaced pairs and scaled to all of them;
  (b) what the project could do before: usip_icp_nearest_f32 (the exact nearest row, whose walk ends only where the x-gap
      exceeds the best distance found) on the same bank, poses and query order, then the two thresholds in torch -- timed on
      `--nearest-pairs` evenly spaced pairs and scaled, its counts checked against the reach kernel's.
One JSON line; --out writes it to a file as well.

    python tools/ground_truth_bench.py [--fragments 57] [--points 400000] [--leaf 0.01] [--batch-pairs 32] [--repeats 3]
                                       [--threads 16] [--host-pairs 64] [--nearest-pairs 96]
                                       [--out profiles/f18_ground_truth_bench.json]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usip_amd import fragments as fr, ground_truth as gtm, ops      # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    return out, (s, e)


def spaced(n, k):
    return np.unique(np.linspace(0, n - 1, max(1, min(k, n))).astype(int))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=57)
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--leaf", type=float, default=gtm.LEAF)
    ap.add_argument("--batch-pairs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=64)
    ap.add_argument("--nearest-pairs", type=int, default=96)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    F = a.fragments
    sc = fr.synthetic_scene(a.seed, F, a.points, 8, ground_truth=False)
    f1h, f2h, trans = gtm.scene_pairs(sc["poses"])
    P = len(f1h)
    gtm.check_voxel_range(sc["clouds"], a.leaf)
    fr.RefineBank(sc["clouds"][:2], "cuda:0", a.leaf)                      # warm-up
    torch.cuda.synchronize()
    bank, ev_bank = timed(lambda: fr.RefineBank(sc["clouds"], "cuda:0", a.leaf))
    f1d, f2d = torch.from_numpy(f1h).cuda(), torch.from_numpy(f2h).cuda()
    Rtd = torch.from_numpy(np.ascontiguousarray(trans[:, :3])).cuda()
    ids = torch.arange(P, dtype=torch.int64, device="cuda")
    names = ("keys_sort", "reach", "selection", "information")

    def run_scene(limit, events, keep):
        for base in range(0, limit, a.batch_pairs):
            sl = slice(base, min(base + a.batch_pairs, P))
            g1, g2, Rt = f1d[sl], f2d[sl], Rtd[sl]
            perm2, ev = timed(lambda: fr.moved_x_order(bank, g2, Rt))
            events["keys_sort"].append(ev)
            o, ev = timed(lambda: ops.gt_reach(bank.rows, bank.offsets, bank.perm, g1, g2, Rt, perm2, gtm.FAR, gtm.NEAR, a.seed,
                                               ids[sl]))
            events["reach"].append(ev)
            order, ev = timed(lambda: gtm.select_rows(o["key"], gtm.CAP))
            events["selection"].append(ev)
            info, ev = timed(lambda: ops.gt_information(bank.rows, bank.offsets, g2, Rt, order, o["hits"][:, 1].contiguous(),
                                                        bank.lmax))
            events["information"].append(ev)
            if keep is not None:
                keep.append((o["hits"], o["ratio"], info))

    run_scene(a.batch_pairs, {k: [] for k in names}, None)                 # warm-up: one batch
    torch.cuda.synchronize()
    per_repeat, walls, kept = {k: [] for k in names}, [], []
    for r in range(a.repeats):
        events = {k: [] for k in names}
        kept = []
        t0 = time.perf_counter()
        run_scene(P, events, kept)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        for k in names:
            per_repeat[k].append(sum(s.elapsed_time(e) for s, e in events[k]))
    stage_ms = {k: float(np.median(v)) for k, v in per_repeat.items()}
    hits, ratio, info = [torch.cat([o[k] for o in kept]).cpu().numpy() for k in range(3)]
    device_ms = sum(stage_ms.values())
    lengths = np.asarray(bank.lengths, np.float64)

    # (b) the exact nearest search, then the thresholds in torch, on evenly spaced pairs
    pick_b = spaced(P, a.nearest_pairs)
    n2 = torch.tensor([bank.lengths[j] for j in f2h], dtype=torch.int64, device="cuda")
    live_row = torch.arange(bank.lmax, device="cuda")[None, :]

    def composition(sel):
        g1, g2, Rt = f1d[sel].contiguous(), f2d[sel].contiguous(), Rtd[sel].contiguous()
        perm2 = fr.moved_x_order(bank, g2, Rt)
        _, d2 = ops.icp_nearest(bank.rows, bank.offsets, bank.perm, g1, g2, Rt, bank.lmax, None, perm2)
        d = torch.sqrt(d2)
        live = live_row < n2[sel][:, None]
        return torch.stack((((d < gtm.FAR) & live).sum(1), ((d < gtm.NEAR) & live).sum(1)), 1)

    sel_b = torch.from_numpy(pick_b).cuda()
    composition(sel_b[:2])                                                 # warm-up
    torch.cuda.synchronize()
    times_b, hits_b = [], None
    for r in range(a.repeats):
        ms = 0.0
        parts = []
        for base in range(0, len(pick_b), a.batch_pairs):
            got, (s, e) = timed(lambda: composition(sel_b[base:base + a.batch_pairs]))
            torch.cuda.synchronize()
            ms += s.elapsed_time(e)
            parts.append(got)
        times_b.append(ms)
        hits_b = torch.cat(parts).cpu().numpy()
    nearest_ms = float(np.median(times_b))
    nearest_equal = bool(np.array_equal(hits_b, hits[pick_b]))
    # the bounded walk on the same picked pairs, for a like-for-like ratio
    times_r = []
    for r in range(a.repeats):
        ms = 0.0
        for base in range(0, len(pick_b), a.batch_pairs):
            sel = sel_b[base:base + a.batch_pairs]
            g1, g2, Rt = f1d[sel].contiguous(), f2d[sel].contiguous(), Rtd[sel].contiguous()
            _, (s, e) = timed(lambda: ops.gt_reach(bank.rows, bank.offsets, bank.perm, g1, g2, Rt, fr.moved_x_order(bank, g2, Rt),
                                                   gtm.FAR, gtm.NEAR, a.seed, ids[sel].contiguous()))
            torch.cuda.synchronize()
            ms += s.elapsed_time(e)
        times_r.append(ms)
    reach_same_pairs_ms = float(np.median(times_r))

    # (a) the host twin on evenly spaced pairs
    pick_a = spaced(P, a.host_pairs)
    host = bank.host()
    t0 = time.perf_counter()
    h = gtm.pairs_ground_truth_cpu(host, f1h[pick_a], f2h[pick_a], trans[pick_a, :3], seed=a.seed,
                                   pair_ids=pick_a.astype(np.int64), batch_pairs=a.batch_pairs, num_threads=a.threads)
    host_ms = (time.perf_counter() - t0) * 1e3
    host_equal = bool(np.array_equal(h["hits"], hits[pick_a])
                      and np.array_equal(h["info"].view(np.uint64), info[pick_a].view(np.uint64))
                      and np.array_equal(h["ratio"].view(np.uint64), ratio[pick_a].view(np.uint64)))
    host_scaled = host_ms * P / len(pick_a)
    written = ratio[:, 0] >= gtm.MIN_RATIO
    res = {"what": "ground_truth_bench",
           "shape": {"fragments": F, "pairs": P, "points_per_fragment": a.points, "leaf": a.leaf, "batch_pairs": a.batch_pairs,
                     "rows_per_averaged_fragment_mean": round(float(lengths.mean()), 1),
                     "rows_per_averaged_fragment_max": int(lengths.max()), "repeats": a.repeats},
           "pairs_written": int(written.sum()), "pairs_with_a_row_within_far": int((hits[:, 0] > 0).sum()),
           "near_rows_mean_of_written": round(float(hits[written, 1].mean()), 1) if written.any() else 0.0,
           "bank_grid_average_ms": round(ev_bank[0].elapsed_time(ev_bank[1]), 2),
           "device_stage_ms_median": {k: round(v, 2) for k, v in stage_ms.items()},
           "device_stage_ms_all_repeats": {k: [round(x, 2) for x in v] for k, v in per_repeat.items()},
           "device_scene_ms": round(device_ms, 2), "wall_s_median": round(float(np.median(walls)), 3),
           "host_twin": {"threads": a.threads, "pairs_timed": int(len(pick_a)), "ms_timed": round(host_ms, 1),
                         "ms_scaled_to_all_pairs": round(host_scaled, 1), "over_device": round(host_scaled / device_ms, 1),
                         "equal_to_device_bit_for_bit": host_equal},
           "exact_nearest_then_thresholds": {"pairs_timed": int(len(pick_b)), "ms_timed_median": round(nearest_ms, 2),
                                             "ms_all_repeats": [round(x, 2) for x in times_b],
                                             "keys_sort_and_reach_on_the_same_pairs_ms_median": round(reach_same_pairs_ms, 2),
                                             "over_bounded_walk_on_the_same_pairs": round(nearest_ms / reach_same_pairs_ms, 2),
                                             "ms_scaled_to_all_pairs": round(nearest_ms * P / len(pick_b), 1),
                                             "counts_equal_to_reach": nearest_equal},
           "device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
