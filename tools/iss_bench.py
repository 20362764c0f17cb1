#!/usr/bin/env python
"""Times of the f-11 ISS baseline detector (usip_amd/baselines.py) at the KITTI shape: B = 8 frames of N = 16384 points,
usip_amd.synth slab clouds, radii 2 / 2, gamma 0.975, min_neighbors 5, 512 keypoints per frame.  Per-stage device time --
(a) the sort along x, (b) the saliency kernel, (c) the suppression kernel, (d) the keypoint selection -- the pair tests the
saliency kernel performs (the tiles its workgroups walk x 256^2, from the counts the kernel writes) and their rate, and the
library's host twin (all pairs) on `--threads` threads.  ONE JSON line, also written to --out.

    python tools/iss_bench.py [--reps 10] [--threads 16] [--skip-host] [--out profiles/f11_iss_bench.json]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows; the whole
detector (IssDetector.__call__ and a synchronise) is timed on the wall clock, median of 5.  No share of a peak is given: a
pair test is about 12 float64 vector operations (3 conversions, 3 subtractions, 3 multiplications, 2 additions, 1 compare)
and one 16-byte LDS broadcast read, and no float64 vector rate of this chip has been published or measured here to hold it
against; operations per second are reported as counted."""
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
from usip_amd import baselines, ops, synth      # noqa: E402

F64_OPS_PER_PAIR_TEST = 12


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
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--num", type=int, default=512)
    ap.add_argument("--skip-host", action="store_true", help="leave the all-pairs host twin out (seconds per call)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f11_iss_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "iss_bench needs a GPU"
    B, N = args.frames, args.points
    rng = np.random.default_rng(11)
    clouds = np.stack([synth.make_cloud(rng, N, "slab") for _ in range(B)]).astype(np.float32)
    pc = torch.from_numpy(clouds).cuda()
    P = dict(baselines.ISS_DEFAULTS)
    rs, rn, g21, g32, mn = (P[k] for k in ("salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors"))
    res = {"metric": "f11_iss", "device": torch.cuda.get_device_name(0), "host": platform.node(), "frames": B, "points": N,
           "keypoints_per_frame": args.num, **P}

    perm = baselines.sort_along_x(pc)
    sal, nb, visits = ops.iss_saliency(pc, None, perm, rs, g21, g32, mn, want_visits=True)
    mask = ops.iss_nms(pc, None, perm, sal, rn, mn)
    tiles = (N + 255) // 256
    pair_tests = float(visits.double().sum()) * 256.0 * 256.0
    res["tiles_visited_share"] = float(visits.double().sum()) / (B * tiles * tiles)
    res["tiles_visited_max_of_%d" % tiles] = int(visits.max())
    res["pair_tests"] = pair_tests
    res["neighbours_mean"] = float(nb.double().mean())
    res["salient_share"] = float((sal > 0).double().mean())
    res["iss_keypoints_per_frame"] = [int(v) for v in mask.sum(1).tolist()]
    u = baselines._draws(B, N, 0, None).cuda()
    stages = {"sort_x_us": lambda: baselines.sort_along_x(pc),
              "saliency_us": lambda: ops.iss_saliency(pc, None, perm, rs, g21, g32, mn),
              "nms_us": lambda: ops.iss_nms(pc, None, perm, sal, rn, mn),
              "selection_us": lambda: baselines._select(pc, mask, None, args.num, True, u)}
    for name, fn in stages.items():
        res[name], res[name + "_all"] = device_us(fn, args.reps)
    res["device_stages_total_ms"] = sum(res[k] for k in stages) * 1e-3
    det = baselines.IssDetector(num=args.num)
    res["detector_wall_ms"] = wall_ms(lambda: (det(pc), torch.cuda.synchronize()))
    res["pair_tests_per_s"] = pair_tests / (res["saliency_us"] * 1e-6)
    res["f64_ops_per_pair_test"] = F64_OPS_PER_PAIR_TEST
    res["f64_ops_per_s"] = F64_OPS_PER_PAIR_TEST * res["pair_tests_per_s"]
    res["share_of_f64_vector_peak"] = None                               # no published or measured rate to hold it against
    if not args.skip_host:
        res["host_threads"] = args.threads
        t0 = time.perf_counter()
        hmask, hsal, hnb = baselines.iss_keypoints_cpu(clouds, None, num_threads=args.threads, **P)
        res["host_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_saliency_pair_tests"] = float(B) * N * N              # (the suppression pass adds N per salient point)
        res["saliency_equals_host_bits"] = bool(np.array_equal(sal.cpu().numpy().view(np.int64), hsal.view(np.int64)))
        res["neighbours_equal_host"] = bool(np.array_equal(nb.cpu().numpy(), hnb))
        res["keypoints_equal_host"] = bool(np.array_equal(mask.cpu().numpy(), hmask))
        res["device_over_host"] = res["detector_wall_ms"] / res["host_all_pairs_ms"]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
