#!/usr/bin/env python
"""Times of the f-12 Fast Global Registration path (usip_amd/fragments.py, registrator "fgr") on one scene of the Redwood
benchmark's size: 57 fragments (1596 pairs) of 100 000 points, D = 128, at 512 and at 1024 keypoints per fragment.  Per
stage -- nearest descriptor in both directions, mutual rows + normalisation + tuple test, the 64 Gauss-Newton steps +
inliers, gather + information matrix, overlap (keys, sort, walk) -- HIP events on the launch stream after a warm-up batch,
summed over all batches; pairs per second end to end; and beside every stage the library's host twins (csrc/fgr_cpu.cpp,
csrc/fragments_cpu.cpp) on `--threads` threads, timed on `--host-pairs` pairs and scaled to the scene.  No ratio to the
reference is claimed: its FGR is a mex file around a library it does not ship.  The RANSAC path's time on the same box is
tools/fragments_bench.py's.  One JSON line; --out writes it to a file as well.

    python tools/fgr_bench.py [--fragments 57] [--points 100000] [--keypoints 512 1024] [--batch-pairs 32] [--threads 16]
                              [--host-pairs 8] [--out profiles/f12_fgr_bench.json]"""
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

STAGES = ("nearest", "tuples", "optimize", "information", "overlap")


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
    nn12, nn21 = clock.run("nearest", lambda: (fr.match_descriptors_topk(d1, d2, n1, n2, 1)[0],
                                               fr.match_descriptors_topk(d2, d1, n2, n1, 1)[0]))
    t = clock.run("tuples", lambda: ops.fgr_tuples(kp1, kp2, n1, n2, nn12, nn21, a.seed, ids))
    o = clock.run("optimize", lambda: ops.fgr_optimize(kp1, kp2, t["mutual"], t["mutual_count"], t["norm"], t["rows"],
                                                       t["row_count"], fr.INLIER_THRESHOLD))

    def information():
        x1 = torch.gather(kp1, 2, t["mutual"][:, :, 0].long().unsqueeze(1).expand(-1, 3, -1)).contiguous()
        return fr.information_matrix(x1, o["inlier_mask"])
    clock.run("information", information)
    ratio, _ = clock.run("overlap", lambda: fr.overlap_ratio(bank, f1, f2, o["Rt"]))
    return o["inliers"], t["mutual_count"], ratio, o["valid"], t["row_count"], t["trials_walked"]


def host_batch(kp1, d1, n1, kp2, d2, n2, bank, f1, f2, ids, a):
    t = {}

    def run(name, fn):
        t0 = time.perf_counter()
        out = fn()
        t[name] = (time.perf_counter() - t0) * 1e3
        return out
    nn12, nn21 = run("nearest", lambda: (fr.match_descriptors_topk_cpu(d1, d2, n1, n2, 1, a.threads)[0],
                                         fr.match_descriptors_topk_cpu(d2, d1, n2, n1, 1, a.threads)[0]))
    tu = run("tuples", lambda: fr.fgr_tuples_cpu(kp1, kp2, n1, n2, nn12, nn21, a.seed, ids, None, 0, a.threads))
    o = run("optimize", lambda: fr.fgr_optimize_cpu(kp1, kp2, tu["mutual"], tu["mutual_count"], tu["norm"], tu["rows"],
                                                    tu["row_count"], fr.INLIER_THRESHOLD, a.threads))
    run("information", lambda: fr.information_matrix_cpu(
        np.ascontiguousarray(np.take_along_axis(kp1, np.broadcast_to(tu["mutual"][:, None, :, 0], kp1.shape), 2)),
        o["inlier_mask"]))
    run("overlap", lambda: fr.overlap_ratio_cpu(bank, f1, f2, o["Rt"], fr.OVERLAP_RADIUS, True, a.threads))
    return t


def one_size(a, M):
    F = a.fragments
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
    inliers, matches, ratio, valid, rows, walked = [torch.cat([o[k] for o in outs]).cpu().numpy() for k in range(6)]

    hp = max(1, min(a.host_pairs, len(pairs)))
    pick = np.linspace(0, len(pairs) - 1, hp).astype(int)                  # near and far pairs alike
    g1, g2 = f1h[pick], f2h[pick]
    host = host_batch(kp[g1], de[g1], cnt[g1], kp[g2], de[g2], cnt[g2], fr.host_bank(sc["clouds"]), g1, g2,
                      pick.astype(np.int64), a)
    scale = len(pairs) / hp
    return {"shape": {"fragments": F, "pairs": len(pairs), "points_per_fragment": a.points, "keypoints": M, "dim": a.dim,
                      "batch_pairs": a.batch_pairs, "mutual_rows_mean": round(float(matches.mean()), 1),
                      "tuple_rows_mean": round(float(rows.mean()), 1), "trials_walked_mean": round(float(walked.mean()), 1)},
            "device_stage_ms": {k: round(v, 2) for k, v in stage_ms.items()},
            "device_total_ms": round(sum(stage_ms.values()), 2), "wall_s": round(wall, 3),
            "pairs_per_s": round(len(pairs) / wall, 1),
            "host_twin": {"threads": a.threads, "pairs_timed": hp,
                          "stage_ms_scaled_to_scene": {k: round(v * scale, 1) for k, v in host.items()},
                          "total_ms_scaled_to_scene": round(sum(host.values()) * scale, 1)},
            "sanity": {"pairs_valid": int((valid != 0).sum()), "pairs_with_inliers": int((inliers > 0).sum()),
                       "pairs_past_gate": int(((ratio[:, 0] > fr.GATE_ALIGNED)
                                               & (inliers / np.maximum(matches, 1) > fr.GATE_INLIER_RATIO)).sum())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=57)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--keypoints", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-pairs", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"what": "fgr_bench", "sizes": {str(M): one_size(a, M) for M in a.keypoints},
           "compared_against": "the library's host twin on %d threads, timed on %d pairs and scaled to the scene; the "
                               "reference's FGR is a mex file around a library it does not ship" % (a.threads, a.host_pairs),
           "device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
