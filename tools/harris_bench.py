#!/usr/bin/env python
"""Times of the f-16 Harris3D baseline detector (usip_amd/baselines.py) at tools/iss_bench.py's shape: B = 8 frames of N = 16384
points, usip_amd.synth slab clouds, radius 1, threshold 0.001, response "harris", 512 keypoints per frame.  Per-stage device
time -- (a) the sort along x, (b) the normals kernel, (c) the response kernel, (d) the suppression (the threshold and f-11's
suppression kernel with min_neighbors 1), (e) the keypoint selection -- the pair tests either kernel performs (the tiles its
workgroups walk x 256^2, from the counts the response kernel writes; the normals kernel walks the same tiles) and their rate,
the library's host twin (all pairs) on `--threads` threads, and, in the same call on the same device, the stages of the ISS
detector at its own defaults.  ONE JSON line, also written to --out.

    python tools/harris_bench.py [--reps 10] [--threads 16] [--skip-host] [--out profiles/f16_harris_bench.json]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows; a whole
detector (its __call__ and a synchronise) is timed on the wall clock, median of 5.  No share of a peak is given, for
tools/iss_bench.py's reason: no float64 vector rate of this chip has been published or measured here to hold a figure against."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from usip_amd import baselines, ops, synth      # noqa: E402
from iss_bench import device_us, wall_ms        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--num", type=int, default=512)
    ap.add_argument("--skip-host", action="store_true", help="leave the all-pairs host twin out (seconds per call)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_harris_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "harris_bench needs a GPU"
    B, N = args.frames, args.points
    rng = np.random.default_rng(11)                                    # (tools/iss_bench.py's clouds)
    clouds = np.stack([synth.make_cloud(rng, N, "slab") for _ in range(B)]).astype(np.float32)
    pc = torch.from_numpy(clouds).cuda()
    P = dict(baselines.HARRIS_DEFAULTS)
    r, thr, method, mn = (P[k] for k in ("radius", "threshold", "response", "min_neighbors"))
    res = {"metric": "f16_harris", "device": torch.cuda.get_device_name(0), "host": platform.node(), "frames": B, "points": N,
           "keypoints_per_frame": args.num, **P}

    perm = baselines.sort_along_x(pc)
    normals, nb = ops.harris_normals(pc, None, perm, r, mn)
    resp, members, visits = ops.harris_response(pc, None, perm, normals, r, method, want_visits=True)

    def suppress():
        return ops.iss_nms(pc, None, perm, torch.where(resp >= thr, resp, torch.zeros_like(resp)), r, 1)

    mask = suppress()
    tiles = (N + 255) // 256
    pair_tests = float(visits.double().sum()) * 256.0 * 256.0
    res["tiles_visited_share"] = float(visits.double().sum()) / (B * tiles * tiles)
    res["tiles_visited_max_of_%d" % tiles] = int(visits.max())
    res["pair_tests_per_kernel"] = pair_tests
    res["neighbours_mean"] = float(nb.double().mean())
    res["with_normal_share"] = float((nb >= mn).double().mean())
    res["at_or_above_threshold_share"] = float(((resp >= thr) & (resp > 0)).double().mean())
    res["harris_keypoints_per_frame"] = [int(v) for v in mask.sum(1).tolist()]
    u = baselines._draws(B, N, 0, None).cuda()
    stages = {"sort_x_us": lambda: baselines.sort_along_x(pc),
              "normals_us": lambda: ops.harris_normals(pc, None, perm, r, mn),
              "response_us": lambda: ops.harris_response(pc, None, perm, normals, r, method),
              "suppression_us": suppress,
              "selection_us": lambda: baselines._select(pc, mask, None, args.num, True, u)}
    for name, fn in stages.items():
        res[name], res[name + "_all"] = device_us(fn, args.reps)
    res["device_stages_total_ms"] = sum(res[k] for k in stages) * 1e-3
    det = baselines.HarrisDetector(num=args.num)
    res["detector_wall_ms"] = wall_ms(lambda: (det(pc), torch.cuda.synchronize()))
    res["normals_pair_tests_per_s"] = pair_tests / (res["normals_us"] * 1e-6)
    res["response_pair_tests_per_s"] = pair_tests / (res["response_us"] * 1e-6)
    res["share_of_f64_vector_peak"] = None                               # no published or measured rate to hold it against

    # ISS at its defaults, same clouds, same device, same call
    I = dict(baselines.ISS_DEFAULTS)
    rs, rn, g21, g32, imn = (I[k] for k in ("salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors"))
    sal, inb, ivis = ops.iss_saliency(pc, None, perm, rs, g21, g32, imn, want_visits=True)
    imask = ops.iss_nms(pc, None, perm, sal, rn, imn)
    iss = {**I, "tiles_visited_share": float(ivis.double().sum()) / (B * tiles * tiles),
           "pair_tests": float(ivis.double().sum()) * 256.0 * 256.0,
           "iss_keypoints_per_frame": [int(v) for v in imask.sum(1).tolist()]}
    istages = {"sort_x_us": lambda: baselines.sort_along_x(pc),
               "saliency_us": lambda: ops.iss_saliency(pc, None, perm, rs, g21, g32, imn),
               "nms_us": lambda: ops.iss_nms(pc, None, perm, sal, rn, imn),
               "selection_us": lambda: baselines._select(pc, imask, None, args.num, True, u)}
    for name, fn in istages.items():
        iss[name], iss[name + "_all"] = device_us(fn, args.reps)
    iss["device_stages_total_ms"] = sum(iss[k] for k in istages) * 1e-3
    idet = baselines.IssDetector(num=args.num)
    iss["detector_wall_ms"] = wall_ms(lambda: (idet(pc), torch.cuda.synchronize()))
    iss["pair_tests_per_s"] = iss["pair_tests"] / (iss["saliency_us"] * 1e-6)
    res["iss_same_call"] = iss

    if not args.skip_host:
        res["host_threads"] = args.threads
        t0 = time.perf_counter()
        hmask, hres, hmem, hnrm = baselines.harris_keypoints_cpu(clouds, None, num_threads=args.threads, **P)
        res["host_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_pair_tests_per_pass"] = float(B) * N * N             # (two passes; the suppression adds N per kept point)
        res["normals_equal_host_bits"] = bool(np.array_equal(normals.cpu().numpy().view(np.int64), hnrm.view(np.int64)))
        res["response_equals_host_bits"] = bool(np.array_equal(resp.cpu().numpy().view(np.int64), hres.view(np.int64)))
        res["members_equal_host"] = bool(np.array_equal(members.cpu().numpy(), hmem))
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
