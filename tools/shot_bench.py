#!/usr/bin/env python
"""Times of the f-20 SHOT baseline descriptor (usip_amd/baselines.py) at tools/fpfh_bench.py's shape: B = 8 frames of N = 16384
points, usip_amd.synth slab clouds, 512 ISS keypoints per frame, radius 2, normal radius 1.  Per-stage device time -- (a) the
sort along x, (b) the normals kernel (f-16's, at the normal radius), (c) the frame kernel, (d) the histogram kernel -- one whole
ShotDescriptor call on the wall clock, FpfhDescriptor's call in the same process, the library's host twin (all pairs) on
`--threads` threads, the mean lrf_members and kp_members and the share of keypoints without a frame.  ONE JSON line, also
written to --out.

    python tools/shot_bench.py [--reps 10] [--threads 16] [--skip-host] [--out profiles/f20_shot_bench.json]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows; a whole
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f20_shot_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "shot_bench needs a GPU"
    B, N, M = args.frames, args.points, args.num
    rng = np.random.default_rng(11)                                    # (tools/iss_bench.py's clouds)
    clouds = np.stack([synth.make_cloud(rng, N, "slab") for _ in range(B)]).astype(np.float32)
    pc = torch.from_numpy(clouds).cuda()
    P = dict(baselines.SHOT_DEFAULTS)
    r, nr, mn = (P[k] for k in ("radius", "normal_radius", "min_neighbors"))
    res = {"metric": "f20_shot", "device": torch.cuda.get_device_name(0), "host": platform.node(), "frames": B, "points": N,
           "keypoints_per_frame": M, **P}

    kp, kp_count = baselines.IssDetector(num=M)(pc)
    perm = baselines.sort_along_x(pc)
    normals, nb = ops.harris_normals(pc, None, perm, nr, mn)
    lrf, lrf_members = ops.shot_lrf(pc, None, perm, kp, kp_count, r)
    hist, shot, kpm = ops.shot_hist(pc, None, perm, normals, kp, kp_count, lrf, r)
    res["with_normal_share"] = float((nb >= mn).double().mean())
    res["lrf_members_mean"] = float(lrf_members.double().mean())
    res["kp_members_mean"] = float(kpm.double().mean())
    res["without_frame_share"] = float((lrf.abs().sum(2) == 0).double().mean())
    res["descriptors_all_zero_share"] = float((shot.abs().sum(2) == 0).double().mean())
    stages = {"sort_x_us": lambda: baselines.sort_along_x(pc),
              "normals_us": lambda: ops.harris_normals(pc, None, perm, nr, mn),
              "lrf_us": lambda: ops.shot_lrf(pc, None, perm, kp, kp_count, r),
              "hist_us": lambda: ops.shot_hist(pc, None, perm, normals, kp, kp_count, lrf, r)}
    for name, fn in stages.items():
        res[name], res[name + "_all"] = device_us(fn, args.reps)
    res["device_stages_total_ms"] = sum(res[k] for k in stages) * 1e-3
    describe = baselines.ShotDescriptor(**P)
    res["descriptor_wall_ms"] = wall_ms(lambda: (describe(pc, kp, None, kp_count), torch.cuda.synchronize()))
    fpfh = baselines.FpfhDescriptor(**baselines.FPFH_DEFAULTS)
    res["fpfh_descriptor_wall_ms"] = wall_ms(lambda: (fpfh(pc, kp, None, kp_count), torch.cuda.synchronize()))
    res["hist_members_per_s"] = float(kpm.double().sum()) / (res["hist_us"] * 1e-6)
    res["share_of_f64_vector_peak"] = None                               # no published or measured rate to hold it against

    if not args.skip_host:
        res["host_threads"] = args.threads
        k, kc = kp.cpu().numpy(), kp_count.cpu().numpy()
        t0 = time.perf_counter()
        hn = baselines.harris_normals_cpu(clouds, None, nr, mn, args.threads)[0]
        res["host_normals_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        hl, hlm = baselines.shot_frames_cpu(clouds, k, None, kc, r, args.threads)
        res["host_lrf_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        hh, hs, hk = baselines.shot_hist_cpu(clouds, None, hn, k, kc, hl, r, args.threads)
        res["host_hist_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_all_pairs_ms"] = sum(res["host_%s_all_pairs_ms" % s] for s in ("normals", "lrf", "hist"))
        res["lrf_equals_host_bits"] = bool(np.array_equal(lrf.cpu().numpy().view(np.int64), hl.view(np.int64))
                                           and np.array_equal(lrf_members.cpu().numpy(), hlm))
        res["hist_equals_host"] = bool(np.array_equal(hist.cpu().numpy(), hh) and np.array_equal(kpm.cpu().numpy(), hk))
        res["shot_equals_host_bits"] = bool(np.array_equal(shot.cpu().numpy().view(np.int64), hs.view(np.int64)))
        res["device_over_host"] = res["descriptor_wall_ms"] / res["host_all_pairs_ms"]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
