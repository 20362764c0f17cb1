#!/usr/bin/env python
"""Times of the f-13 refinement (usip_amd/fragments.py: RefineBank, icp_refine) on the scene of tools/fgr_bench.py: 57
fragments (1596 pairs) of 100 000 points, D = 128, 512 keypoints per fragment, registered by Fast Global Registration.
Per stage, HIP events summed over the scene: the downsampling of the fragments (once), the moved-x keys and their sort,
and -- from the library's own events between its launches -- the nearest, trim and fit launches of the loop and the final
pass; the number of pairs refined (mask = valid & inlier_ratio > 0.025), the mean rows per downsampled fragment, the mean
iterations of the refined pairs and the share of their n1 n2 (query, row) distances that the lanes evaluated per pass.  Beside
it, in the same run: the full-cloud overlap walk of the same pairs, and the library's host twin (csrc/icp_cpu.cpp, whose
search is the loop over all rows) on `--threads` threads, timed on `--host-pairs` of the refined pairs and scaled to them.
One JSON line; --out writes it to a file as well.

--metric plane times the same stages under the point-to-plane metric (f-28): the bank is built with normals (the downsampling
stage then includes them), the loop runs icp_fit_plane_kernel, and -- in the same process, after it, on the same bank and
estimates -- the point-to-point loop runs once more, so that "beside_point_to_point" holds the other fit's stage times and
iterations per pair next to this one's.

    python tools/icp_bench.py [--fragments 57] [--points 100000] [--keypoints 512] [--batch-pairs 32] [--threads 16]
                              [--host-pairs 8] [--metric point|plane] [--out profiles/f13_icp_bench.json]"""
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


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    return out, (s, e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=57)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-pairs", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--metric", choices=("point", "plane"), default="point")
    ap.add_argument("--out")
    a = ap.parse_args()
    metric = {"point": "point_to_point", "plane": "point_to_plane"}[a.metric]
    plane = a.metric == "plane"
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
    fr.RefineBank(sc["clouds"][:2], "cuda:0", normals=plane)               # warm-up
    torch.cuda.synchronize()
    fine, ev_down = timed(lambda: fr.RefineBank(sc["clouds"], "cuda:0", normals=plane))
    dkp, dde, dcnt = [torch.from_numpy(t).cuda() for t in (kp, de, cnt)]
    f1d, f2d = torch.from_numpy(f1h).cuda(), torch.from_numpy(f2h).cuda()
    ir, it, tt, tc, ar = fr._refine_args(fr.REFINE_INLIER_RATIO, fr.REFINE_ITERATIONS, fr.REFINE_TOLERANCE, fr.REFINE_RADIUS)

    events = {"keys_sort": [], "overlap": [], "register": []}
    stage = np.zeros(4)
    outs = []

    def run_all(limit=None, measure=True, metric=metric, stage=stage, outs=outs):
        for base in range(0, len(pairs) if limit is None else limit, a.batch_pairs):
            sl = slice(base, min(base + a.batch_pairs, len(pairs)))
            i1, i2 = f1d[sl].long(), f2d[sl].long()
            g1, g2 = f1d[sl].contiguous(), f2d[sl].contiguous()
            ids = torch.arange(sl.start, sl.stop, dtype=torch.int64, device="cuda")

            def register():
                nn12, _ = fr.match_descriptors_topk(dde[i1], dde[i2], dcnt[i1].contiguous(), dcnt[i2].contiguous(), 1)
                nn21, _ = fr.match_descriptors_topk(dde[i2], dde[i1], dcnt[i2].contiguous(), dcnt[i1].contiguous(), 1)
                return fr.fgr_registration(dkp[i1].contiguous(), dkp[i2].contiguous(), dcnt[i1].contiguous(),
                                           dcnt[i2].contiguous(), nn12, nn21, fr.INLIER_THRESHOLD, a.seed, ids)
            reg, ev = timed(register)
            events["register"].append(ev)
            Rt = reg.Rt.contiguous()
            mask = ((reg.valid != 0) & (reg.inlier_ratio > fr.GATE_INLIER_RATIO)).to(torch.uint8).contiguous()
            (ratio, _), ev = timed(lambda: fr.overlap_ratio(bank, g1, g2, Rt))
            events["overlap"].append(ev)
            order2, ev = timed(lambda: torch.argsort(ops.overlap_keys(fine.rows, fine.offsets, g2, Rt, fine.lmax), dim=1,
                                                     stable=True).to(torch.int32))
            events["keys_sort"].append(ev)
            o = ops.icp_refine(fine.rows, fine.offsets, fine.perm, g1, g2, Rt, fine.lmax, mask, order2, ir, it, tt, tc, ar,
                               want_visits=True, want_stage_ms=measure, metric=metric)
            if measure:
                stage[:] += o["stage_ms"]
                outs.append((mask, o["iterations"], o["converged"], o["visits"], o["ratio"], ratio, reg.inlier_ratio, Rt, o["Rt"]))

    run_all(a.batch_pairs, False)                                          # warm-up: one batch
    torch.cuda.synchronize()
    for v in events.values():
        v.clear()
    t0 = time.perf_counter()
    run_all()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = {k: sum(s.elapsed_time(e) for s, e in v) for k, v in events.items()}
    beside = None
    if plane:                                                              # the other fit, same process, same bank and estimates
        stage_pt, outs_pt = np.zeros(4), []
        run_all(a.batch_pairs, False, "point_to_point")
        torch.cuda.synchronize()
        run_all(None, True, "point_to_point", stage_pt, outs_pt)
        torch.cuda.synchronize()
        m_pt, it_pt, conv_pt = [torch.cat([o[k] for o in outs_pt]).cpu().numpy() for k in range(3)]
        beside = {"device_stage_ms": {"nearest": round(stage_pt[0], 2), "trim": round(stage_pt[1], 2), "fit": round(stage_pt[2], 2),
                                      "final_pass": round(stage_pt[3], 2)},
                  "iterations_mean": round(float(it_pt[m_pt != 0].mean()), 2) if (m_pt != 0).any() else 0,
                  "pairs_converged": int(conv_pt[m_pt != 0].sum())}
    mask, iters, conv, visits, ratio_ref, ratio_full, inl, Rt0, Rt1 = [torch.cat([o[k] for o in outs]).cpu().numpy() for k in range(9)]
    refined = mask != 0
    lengths = np.asarray(fine.lengths, np.float64)
    n1n2 = lengths[f1h] * lengths[f2h]
    passes = iters.astype(np.float64) + 1.0
    share = float(visits[refined].sum() / (n1n2[refined] * passes[refined]).sum()) if refined.any() else 0.0

    # the host twin on a few of the refined pairs, scaled to all of them
    host_bank = fine.host()
    pick = np.nonzero(refined)[0]
    pick = pick[np.linspace(0, len(pick) - 1, max(1, min(a.host_pairs, len(pick)))).astype(int)] if len(pick) else pick
    host_ms = 0.0
    if len(pick):
        t0 = time.perf_counter()
        h = fr.icp_refine_cpu(host_bank, f1h[pick], f2h[pick], Rt0[pick], None, num_threads=a.threads, metric=metric)
        host_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(h.iterations, iters[pick]) and np.array_equal(h.Rt.view(np.uint64), Rt1[pick].view(np.uint64))
    device_ms = float(stage.sum())
    host_scaled = host_ms * int(refined.sum()) / max(len(pick), 1)
    res = {"what": "icp_bench", "metric": metric,
           "shape": {"fragments": F, "pairs": len(pairs), "points_per_fragment": a.points, "keypoints": M,
                     "batch_pairs": a.batch_pairs, "leaf": fr.REFINE_LEAF, "rows_per_downsampled_fragment_mean":
                     round(float(lengths.mean()), 1), "rows_per_downsampled_fragment_max": int(lengths.max())},
           "pairs_refined": int(refined.sum()), "iterations_mean": round(float(iters[refined].mean()), 2) if refined.any() else 0,
           "pairs_converged": int(conv[refined].sum()), "share_of_n1_n2_distances_evaluated_per_pass": round(share, 4),
           "device_stage_ms": {"downsample": round(ev_down[0].elapsed_time(ev_down[1]), 2), "keys_sort": round(ms["keys_sort"], 2),
                               "nearest": round(stage[0], 2), "trim": round(stage[1], 2), "fit": round(stage[2], 2),
                               "final_pass": round(stage[3], 2)},
           "device_refine_ms": round(device_ms + ms["keys_sort"], 2),
           "same_run": {"fgr_registration_ms": round(ms["register"], 2), "overlap_walk_ms": round(ms["overlap"], 2),
                        "refine_over_overlap_walk": round((device_ms + ms["keys_sort"]) / ms["overlap"], 3)},
           "wall_s": round(wall, 3),
           "host_twin": {"threads": a.threads, "pairs_timed": int(len(pick)), "ms_scaled_to_refined_pairs": round(host_scaled, 1),
                         "over_device": round(host_scaled / device_ms, 1) if device_ms > 0 else None,
                         "equal_to_device_bit_for_bit": True},
           "gates": {"first_gate": int(((ratio_full[:, 0] > fr.GATE_ALIGNED) & (inl > fr.GATE_INLIER_RATIO)).sum()),
                     "refined_gate": int(((ratio_ref[:, 0] > fr.GATE_REFINED) & (inl > fr.GATE_INLIER_RATIO)).sum())},
           "device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine()}
    if beside is not None:
        res["beside_point_to_point"] = beside
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
