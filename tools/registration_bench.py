#!/usr/bin/env python
"""Times of the f-6 evaluation kernels (usip_amd/evaluation.py) at P pairs of `count` matched keypoints and T RANSAC trials:
(a) descriptor matching, (b) the trial kernel, (c) selection + refit, (d) repeatability -- next to the library's host twin
on `--threads` threads, the numpy oracle (tests/eval_oracle.py) and the detector + descriptor eval forward of the same
frames, so a reader sees what share of an evaluation pass RANSAC is.  One JSON line.

    python tools/registration_bench.py [--pairs 8 64] [--count 512] [--trials 10000] [--reps 20]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tests", "examples"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import eval_oracle as eo                        # noqa: E402
import evaluate_registration as ex             # noqa: E402
from usip_amd import evaluation as ev, ops      # noqa: E402


def device_us(fn, reps, windows=5, warmup=3):
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
    return float(np.median(out)), [round(v, 2) for v in out]


def host_ms(fn, reps=3):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def case(P, n, T, C, reps, threads):
    x1, x2, count, gt, _ = eo.make_batch(100 + P, P=P, n=n, T=1)
    rng = np.random.default_rng(P)
    desc = rng.normal(size=(2, P, C, n))
    desc = (desc / np.linalg.norm(desc, axis=2, keepdims=True)).astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    dx1, dx2, dc, dgt, da, dp = d(x1), d(x2), d(count), d(gt), d(desc[0]), d(desc[1])
    ids = torch.arange(P, dtype=torch.int64, device="cuda")
    counts = ops.ransac_trials(dx1, dx2, dc, T, 1.0, 0, ids)[0]
    sel = ops.ransac_select(dx1, dx2, dc, counts, T - 1, 1.0, 0, ids, None, dgt)
    out = {"pairs": P, "count": n, "trials": T, "descriptor_len": C,
           "trialcount_mean": float(sel["trialcount"].double().mean()), "delta_t_max": float(sel["delta_t"].max())}
    out["match_us"], out["match_us_all"] = device_us(lambda: ev.match_descriptors(da, dp, dc, dc), reps)
    out["trials_us"], out["trials_us_all"] = device_us(lambda: ops.ransac_trials(dx1, dx2, dc, T, 1.0, 0, ids), reps)
    out["select_refit_us"], out["select_refit_us_all"] = device_us(
        lambda: ops.ransac_select(dx1, dx2, dc, counts, T - 1, 1.0, 0, ids, None, dgt), reps)
    # the rule's worst case: no trial ends the loop early (scores of 5 %: the budget stays above T)
    low = torch.clamp(counts, max=n // 20)
    out["select_refit_full_scan_us"], _ = device_us(
        lambda: ops.ransac_select(dx1, dx2, dc, low, T - 1, 1.0, 0, ids, None, dgt), reps)
    out["repeatability_us"], out["repeatability_us_all"] = device_us(
        lambda: ev.repeatability(dx1, dc, dx2, dc, dgt, 0.5), reps)
    out["device_total_us"] = out["match_us"] + out["trials_us"] + out["select_refit_us"] + out["repeatability_us"]
    out["trial_fits_per_s"] = P * T / (out["trials_us"] * 1e-6)
    out["trial_residuals_per_s"] = P * T * n / (out["trials_us"] * 1e-6)
    # host twin
    hc = ev.ransac_trials_cpu(x1, x2, count, T, 1.0, 0, np.arange(P), None, threads)[0]
    assert np.array_equal(hc, counts.cpu().numpy())
    out["host_threads"] = threads
    out["host_trials_ms"] = host_ms(lambda: ev.ransac_trials_cpu(x1, x2, count, T, 1.0, 0, np.arange(P), None, threads))
    out["host_trials_ms_1thread"] = host_ms(lambda: ev.ransac_trials_cpu(x1[:1], x2[:1], count[:1], T, 1.0), 1) * P
    out["host_select_refit_ms"] = host_ms(lambda: ev.ransac_select_cpu(x1, x2, count, hc, T - 1, 1.0, 0, np.arange(P), None, gt))
    out["host_match_ms"] = host_ms(lambda: ev.match_descriptors_cpu(desc[0], desc[1], count, count), 1)
    out["host_repeatability_ms"] = host_ms(lambda: ev.repeatability_cpu(x1, count, x2, count, gt, 0.5))
    out["host_total_ms"] = (out["host_trials_ms"] + out["host_select_refit_ms"] + out["host_match_ms"] +
                            out["host_repeatability_ms"])
    out["device_over_host"] = out["device_total_us"] * 1e-3 / out["host_total_ms"]
    # numpy oracle: 200 trials of one pair, scaled (it is a per-trial Python loop)
    tri = np.stack([rng.choice(n, 3, replace=False) for _ in range(200)])
    t0 = time.perf_counter()
    for t in tri:
        eo.trial(x1[0], x2[0], t, 1.0)
    out["oracle_trials_ms_scaled_from_200"] = (time.perf_counter() - t0) * 1e3 / 200 * T * P
    return out


def forward_ms(frames, n, nodes, top):
    rng = np.random.default_rng(1)
    evaluator = ex.build_evaluator("ball", None, top, 1.0, 100, 0)
    scans, _ = ex.make_synthetic(rng, frames, n)
    ex.add_scans(evaluator, scans[:1], nodes, 0)                  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ex.add_scans(evaluator, scans, nodes, 0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--trials", type=int, default=10000)
    ap.add_argument("--descriptor-len", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "registration_bench needs a GPU"
    res = {"metric": "f6_registration", "device": torch.cuda.get_device_name(0), "host": platform.node(),
           "cases": [case(P, args.count, args.trials, args.descriptor_len, args.reps, args.threads) for P in args.pairs]}
    per_frame = forward_ms(args.frames, 16384, 512, args.count)
    res["detector_descriptor_forward_ms_per_frame"] = per_frame
    for c in res["cases"]:
        fwd = 2 * c["pairs"] * per_frame
        c["forward_ms_2P_frames"] = fwd
        c["ransac_share_of_pass"] = (c["trials_us"] + c["select_refit_us"]) * 1e-3 / (fwd + c["device_total_us"] * 1e-3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
