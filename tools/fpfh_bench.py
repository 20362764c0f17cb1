#!/usr/bin/env python
"""Times of the f-19 FPFH baseline descriptor (usip_amd/baselines.py) at tools/iss_bench.py's shape: B = 8 frames of N = 16384
points, usip_amd.synth slab clouds, 512 ISS keypoints per frame, radius 2, normal radius 1.  Per-stage device time -- (a) the
sort along x, (b) the normals kernel (f-16's, at the normal radius), (c) the SPFH pass, (d) the gather at the keypoints -- the
pair tests the SPFH pass performs (the tiles its workgroups walk x 256^2, from the counts it writes) and their rate, one whole
FpfhDescriptor call on the wall clock, the library's host twin (all pairs) on `--threads` threads, and, in the same call on the
same device, the ISS saliency kernel's pair-test rate at its own defaults.  ONE JSON line, also written to --out.

    python tools/fpfh_bench.py [--reps 10] [--threads 16] [--skip-host] [--out profiles/f19_fpfh_bench.json]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows; the whole
descriptor (its __call__ and a synchronise) is timed on the wall clock, median of 5.  No share of a peak is given, for
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f19_fpfh_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fpfh_bench needs a GPU"
    B, N, M = args.frames, args.points, args.num
    rng = np.random.default_rng(11)                                    # (tools/iss_bench.py's clouds)
    clouds = np.stack([synth.make_cloud(rng, N, "slab") for _ in range(B)]).astype(np.float32)
    pc = torch.from_numpy(clouds).cuda()
    P = dict(baselines.FPFH_DEFAULTS)
    r, nr, mn = (P[k] for k in ("radius", "normal_radius", "min_neighbors"))
    res = {"metric": "f19_fpfh", "device": torch.cuda.get_device_name(0), "host": platform.node(), "frames": B, "points": N,
           "keypoints_per_frame": M, **P}

    kp, kp_count = baselines.IssDetector(num=M)(pc)
    perm = baselines.sort_along_x(pc)
    normals, nb = ops.harris_normals(pc, None, perm, nr, mn)
    spfh, members, visits = ops.fpfh_spfh(pc, None, perm, normals, r, want_visits=True)
    fpfh, kpm = ops.fpfh_gather(pc, None, perm, spfh, members, kp, kp_count, r)
    tiles = (N + 255) // 256
    pair_tests = float(visits.double().sum()) * 256.0 * 256.0
    res["tiles_visited_share"] = float(visits.double().sum()) / (B * tiles * tiles)
    res["tiles_visited_max_of_%d" % tiles] = int(visits.max())
    res["spfh_pair_tests"] = pair_tests
    res["with_normal_share"] = float((nb >= mn).double().mean())
    res["members_mean"] = float(members.double().mean())
    res["kp_members_mean"] = float(kpm.double().mean())
    res["descriptors_all_zero_share"] = float((fpfh.abs().sum(2) == 0).double().mean())
    stages = {"sort_x_us": lambda: baselines.sort_along_x(pc),
              "normals_us": lambda: ops.harris_normals(pc, None, perm, nr, mn),
              "spfh_us": lambda: ops.fpfh_spfh(pc, None, perm, normals, r),
              "gather_us": lambda: ops.fpfh_gather(pc, None, perm, spfh, members, kp, kp_count, r)}
    for name, fn in stages.items():
        res[name], res[name + "_all"] = device_us(fn, args.reps)
    res["device_stages_total_ms"] = sum(res[k] for k in stages) * 1e-3
    describe = baselines.FpfhDescriptor(**P)
    res["descriptor_wall_ms"] = wall_ms(lambda: (describe(pc, kp, None, kp_count), torch.cuda.synchronize()))
    res["spfh_pair_tests_per_s"] = pair_tests / (res["spfh_us"] * 1e-6)
    res["spfh_member_pairs_per_s"] = float(members.double().sum()) / (res["spfh_us"] * 1e-6)
    res["share_of_f64_vector_peak"] = None                               # no published or measured rate to hold it against

    # ISS's saliency kernel at its defaults, same clouds, same device, same call
    I = dict(baselines.ISS_DEFAULTS)
    rs, g21, g32, imn = (I[k] for k in ("salient_radius", "gamma_21", "gamma_32", "min_neighbors"))
    sal, inb, ivis = ops.iss_saliency(pc, None, perm, rs, g21, g32, imn, want_visits=True)
    iss = {**I, "pair_tests": float(ivis.double().sum()) * 256.0 * 256.0}
    iss["saliency_us"], iss["saliency_us_all"] = device_us(lambda: ops.iss_saliency(pc, None, perm, rs, g21, g32, imn), args.reps)
    iss["pair_tests_per_s"] = iss["pair_tests"] / (iss["saliency_us"] * 1e-6)
    res["iss_same_call"] = iss

    if not args.skip_host:
        res["host_threads"] = args.threads
        k, kc = kp.cpu().numpy(), kp_count.cpu().numpy()
        t0 = time.perf_counter()
        hs, hm, hn = baselines.fpfh_spfh_cpu(clouds, None, r, None, nr, mn, args.threads)
        res["host_normals_and_spfh_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        hf, hk = baselines.fpfh_gather_cpu(clouds, None, hs, hm, k, kc, r, args.threads)
        res["host_gather_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_all_pairs_ms"] = res["host_normals_and_spfh_all_pairs_ms"] + res["host_gather_all_pairs_ms"]
        res["spfh_equals_host"] = bool(np.array_equal(spfh.cpu().numpy(), hs) and np.array_equal(members.cpu().numpy(), hm))
        res["fpfh_equals_host_bits"] = bool(np.array_equal(fpfh.cpu().numpy().view(np.int64), hf.view(np.int64)))
        res["kp_members_equal_host"] = bool(np.array_equal(kpm.cpu().numpy(), hk))
        res["device_over_host"] = res["descriptor_wall_ms"] / res["host_all_pairs_ms"]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
