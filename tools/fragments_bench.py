#!/usr/bin/env python
"""Times of the f-9 fragment-registration path (usip_amd/fragments.py) on one scene of the Redwood benchmark's size:
57 fragments (1596 pairs) of 100 000 points, 512 keypoints, D = 128, k = 5, 30 000 RANSAC trials.  Per stage -- top-k
matching in both directions, union, gather, trial scores, selection + refit, information matrix, overlap (keys, sort,
walk) -- HIP events on the launch stream after a warm-up batch, summed over all batches; pairs per second end to end;
and beside every stage the library's host twins (csrc/fragments_cpu.cpp, csrc/registration_cpu.cpp) on `--threads` threads, timed on `--host-pairs`
pairs and scaled to the scene.  The host twin is what each device figure is compared against: the reference runs this
path in MATLAB, which cannot be run here, so no ratio to it is claimed.  One JSON line; --out writes it to a file as well.

    python tools/fragments_bench.py [--fragments 57] [--points 100000] [--keypoints 512] [--trials 30000]
                                    [--batch-pairs 32] [--threads 16] [--host-pairs 4] [--out profiles/f9_fragments_bench.json]"""
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
from usip_amd import fragments as fr, ops      # noqa: E402

STAGES = ("topk", "union", "gather", "trials", "select", "information", "overlap")


class StageClock:
    def __init__(self):
        self.marks = []

    def run(self, name, fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        self.marks.append((name, s, e))
        return out

    def totals(self):
        torch.cuda.synchronize()
        out = {k: 0.0 for k in STAGES}
        for name, s, e in self.marks:
            out[name] += s.elapsed_time(e)
        return out


def device_batch(clock, kp1, d1, n1, kp2, d2, n2, bank, f1, f2, ids, a):
    nn12, nn21 = clock.run("topk", lambda: (fr.match_descriptors_topk(d1, d2, n1, n2, a.k)[0],
                                            fr.match_descriptors_topk(d2, d1, n2, n1, a.k)[0]))
    pairs, count = clock.run("union", lambda: fr.match_union(nn12, nn21, n1, n2))

    def gather():
        i1 = pairs[:, :, 0].long().unsqueeze(1).expand(-1, 3, -1)
        i2 = pairs[:, :, 1].long().unsqueeze(1).expand(-1, 3, -1)
        return torch.gather(kp1, 2, i1).contiguous(), torch.gather(kp2, 2, i2).contiguous()
    x1, x2 = clock.run("gather", gather)
    T = a.trials + 1
    counts = clock.run("trials", lambda: ops.ransac_trials_large(x1, x2, count, T, fr.INLIER_THRESHOLD, a.seed, ids)[0])
    o = clock.run("select", lambda: ops.ransac_select_large(x1, x2, count, counts, a.trials, fr.INLIER_THRESHOLD, a.seed, ids))
    clock.run("information", lambda: fr.information_matrix(x1, o["inlier_mask"]))
    eye = torch.eye(3, 4, dtype=torch.float64, device=x1.device)
    Rt = torch.where(o["valid"].reshape(-1, 1, 1) != 0, o["Rt"], eye)
    ratio, _ = clock.run("overlap", lambda: fr.overlap_ratio(bank, f1, f2, Rt))
    return o["inliers"], count, ratio


def host_batch(kp1, d1, n1, kp2, d2, n2, bank, f1, f2, ids, a):
    t = {}

    def run(name, fn):
        t0 = time.perf_counter()
        out = fn()
        t[name] = (time.perf_counter() - t0) * 1e3
        return out
    nn12, nn21 = run("topk", lambda: (fr.match_descriptors_topk_cpu(d1, d2, n1, n2, a.k, a.threads)[0],
                                      fr.match_descriptors_topk_cpu(d2, d1, n2, n1, a.k, a.threads)[0]))
    pairs, count = run("union", lambda: fr.match_union_cpu(nn12, nn21, n1, n2))
    P, C = pairs.shape[:2]
    x1, x2 = run("gather", lambda: (
        np.ascontiguousarray(np.take_along_axis(kp1, np.broadcast_to(pairs[:, None, :, 0], (P, 3, C)), 2)),
        np.ascontiguousarray(np.take_along_axis(kp2, np.broadcast_to(pairs[:, None, :, 1], (P, 3, C)), 2))))
    counts = run("trials", lambda: fr.ransac_trials_large_cpu(x1, x2, count, a.trials + 1, fr.INLIER_THRESHOLD, a.seed, ids,
                                                              None, a.threads)[0])
    o = run("select", lambda: fr.ransac_select_large_cpu(x1, x2, count, counts, a.trials, fr.INLIER_THRESHOLD, a.seed, ids))
    run("information", lambda: fr.information_matrix_cpu(x1, o["inlier_mask"]))
    Rt = np.where(o["valid"].reshape(-1, 1, 1) != 0, o["Rt"], np.eye(3, 4))
    run("overlap", lambda: fr.overlap_ratio_cpu(bank, f1, f2, Rt, fr.OVERLAP_RADIUS, True, a.threads))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=57)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=fr.K_MATCH)
    ap.add_argument("--trials", type=int, default=fr.MAX_TRIALS)
    ap.add_argument("--batch-pairs", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    F, M = a.fragments, a.keypoints
    span, step = 5.0, 1.0
    marks = int(round(M * (span + (F - 1) * step) / span))
    sc = fr.synthetic_scene(a.seed, F, a.points, a.dim, span, step, landmarks=marks, ground_truth=False)
    kp, de, cnt = np.zeros((F, 3, M), np.float32), np.zeros((F, a.dim, M), np.float32), np.zeros(F, np.int32)
    for i in range(F):
        n = min(len(sc["xyz"][i]), M)
        kp[i, :, :n], de[i, :, :n], cnt[i] = sc["xyz"][i][:n].T, sc["desc"][i][:n].T, n
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    f1h, f2h = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    bank = fr.FragmentBank(sc["clouds"], "cuda:0")
    dkp, dde, dcnt = [torch.from_numpy(t).cuda() for t in (kp, de, cnt)]
    f1d, f2d = torch.from_numpy(f1h).cuda(), torch.from_numpy(f2h).cuda()

    def run_all(clock, limit=None):
        outs = []
        for base in range(0, len(pairs) if limit is None else limit, a.batch_pairs):
            sl = slice(base, min(base + a.batch_pairs, len(pairs)))
            i1, i2 = f1d[sl].long(), f2d[sl].long()
            ids = torch.arange(sl.start, sl.stop, dtype=torch.int64, device="cuda")
            outs.append(device_batch(clock, dkp[i1], dde[i1], dcnt[i1].contiguous(), dkp[i2], dde[i2], dcnt[i2].contiguous(),
                                     bank, f1d[sl].contiguous(), f2d[sl].contiguous(), ids, a))
        return outs
    run_all(StageClock(), a.batch_pairs)                                  # warm-up: one batch
    torch.cuda.synchronize()
    clock = StageClock()
    t0 = time.perf_counter()
    outs = run_all(clock)
    stage_ms = clock.totals()
    wall = time.perf_counter() - t0
    inliers = torch.cat([o[0] for o in outs]).cpu().numpy()
    matches = torch.cat([o[1] for o in outs]).cpu().numpy()
    ratio = torch.cat([o[2] for o in outs]).cpu().numpy()

    hp = max(1, min(a.host_pairs, len(pairs)))
    pick = np.linspace(0, len(pairs) - 1, hp).astype(int)                  # near and far pairs alike
    g1, g2 = f1h[pick], f2h[pick]
    host = host_batch(kp[g1], de[g1], cnt[g1], kp[g2], de[g2], cnt[g2], fr.host_bank(sc["clouds"]), g1, g2,
                      pick.astype(np.int64), a)
    scale = len(pairs) / hp
    res = {"what": "fragments_bench", "shape": {"fragments": F, "pairs": len(pairs), "points_per_fragment": a.points,
                                                "keypoints": M, "dim": a.dim, "k": a.k, "trials": a.trials,
                                                "batch_pairs": a.batch_pairs,
                                                "correspondences_mean": round(float(matches.mean()), 1)},
           "device_stage_ms": {k: round(v, 2) for k, v in stage_ms.items()},
           "device_total_ms": round(sum(stage_ms.values()), 2), "wall_s": round(wall, 3),
           "pairs_per_s": round(len(pairs) / wall, 1),
           "host_twin": {"threads": a.threads, "pairs_timed": hp,
                         "stage_ms_scaled_to_scene": {k: round(v * scale, 1) for k, v in host.items()},
                         "total_ms_scaled_to_scene": round(sum(host.values()) * scale, 1)},
           "compared_against": "the library's host twin on %d threads, timed on %d pairs and scaled to %d; the reference's "
                               "MATLAB cannot be run here" % (a.threads, hp, len(pairs)),
           "sanity": {"pairs_with_inliers": int((inliers > 0).sum()),
                      "pairs_past_gate": int(((ratio[:, 0] > fr.GATE_ALIGNED) & (inliers / np.maximum(matches, 1) > fr.GATE_INLIER_RATIO)).sum())},
           "device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
