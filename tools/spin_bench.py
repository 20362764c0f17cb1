#!/usr/bin/env python
"""Times of the f-21 spin-image baseline descriptor (usip_amd/baselines.py) at tools/shot_bench.py's shape: B = 8 frames of N =
16384 points, usip_amd.synth slab clouds, 512 ISS keypoints per frame, radius 2, axis radius 2.  Per-stage device time -- (a)
the sort along x, (b) SHOT's frame kernel, whose z row is the axis, (c) the image kernel, and with --support-angle-cos > 0 (d)
the normals kernel (f-16's, at the normal radius) -- one whole SpinDescriptor call on the wall clock, ShotDescriptor's call and
SHOT's histogram kernel in the same process, the library's host twin (all pairs) on `--threads` threads, the mean members per
keypoint and the share of all-zero rows.  ONE JSON line, also written to --out.

    python tools/spin_bench.py [--structure radial] [--support-angle-cos 0.5] [--reps 10] [--threads 16] [--skip-host]
                               [--out profiles/f21_spin_bench.json]

Device times: events on the launch stream around `reps` back-to-back calls after a warm-up, median of 5 windows; a whole
descriptor (its __call__ and a synchronise) is timed on the wall clock, median of 5.  The image kernel is timed in BOTH
structures whichever one --structure names.  No share of a peak is given, for tools/iss_bench.py's reason."""
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
    ap.add_argument("--structure", default="rectangular", choices=sorted(ops.SPIN_STRUCTURES))
    ap.add_argument("--support-angle-cos", type=float, default=0.0)
    ap.add_argument("--skip-host", action="store_true", help="leave the all-pairs host twin out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f21_spin_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spin_bench needs a GPU"
    B, N, M = args.frames, args.points, args.num
    rng = np.random.default_rng(11)                                    # (tools/iss_bench.py's clouds)
    clouds = np.stack([synth.make_cloud(rng, N, "slab") for _ in range(B)]).astype(np.float32)
    pc = torch.from_numpy(clouds).cuda()
    P = dict(baselines.SPIN_DEFAULTS, structure=args.structure, support_angle_cos=args.support_angle_cos)
    r, nr, mn, s, st = (P[k] for k in ("radius", "normal_radius", "min_neighbors", "support_angle_cos", "structure"))
    res = {"metric": "f21_spin", "device": torch.cuda.get_device_name(0), "host": platform.node(), "frames": B, "points": N,
           "keypoints_per_frame": M, **P}

    kp, kp_count = baselines.IssDetector(num=M)(pc)
    perm = baselines.sort_along_x(pc)
    normals = ops.harris_normals(pc, None, perm, nr, mn)[0] if s > 0.0 else None
    lrf, lrf_members = ops.shot_lrf(pc, None, perm, kp, kp_count, r)
    axes = lrf[:, :, 6:9].contiguous()
    hist, spin, kpm = ops.spin_image(pc, None, perm, normals, kp, kp_count, axes, r, s, st)
    res["lrf_members_mean"] = float(lrf_members.double().mean())
    res["kp_members_mean"] = float(kpm.double().mean())
    res["without_axis_share"] = float((axes.abs().sum(2) == 0).double().mean())
    res["descriptors_all_zero_share"] = float((spin.abs().sum(2) == 0).double().mean())
    stages = {"sort_x_us": lambda: baselines.sort_along_x(pc),
              "lrf_us": lambda: ops.shot_lrf(pc, None, perm, kp, kp_count, r),
              "image_us": lambda: ops.spin_image(pc, None, perm, normals, kp, kp_count, axes, r, s, st)}
    if s > 0.0:
        stages["normals_us"] = lambda: ops.harris_normals(pc, None, perm, nr, mn)
    for name, fn in stages.items():
        res[name], res[name + "_all"] = device_us(fn, args.reps)
    res["device_stages_total_ms"] = sum(res[k] for k in stages) * 1e-3
    for other in sorted(ops.SPIN_STRUCTURES):                          # the image kernel alone, in either structure
        k2 = ops.spin_image(pc, None, perm, normals, kp, kp_count, axes, r, s, other)[2]
        res["image_%s_us" % other] = device_us(lambda: ops.spin_image(pc, None, perm, normals, kp, kp_count, axes, r, s, other),
                                               args.reps)[0]
        res["kp_members_mean_%s" % other] = float(k2.double().mean())
    describe = baselines.SpinDescriptor(**P)
    res["descriptor_wall_ms"] = wall_ms(lambda: (describe(pc, kp, None, kp_count), torch.cuda.synchronize()))
    # the yardstick: SHOT in the same process -- its whole call, and its histogram kernel over the same window
    shot = baselines.ShotDescriptor(**baselines.SHOT_DEFAULTS)
    res["shot_descriptor_wall_ms"] = wall_ms(lambda: (shot(pc, kp, None, kp_count), torch.cuda.synchronize()))
    shot_normals = ops.harris_normals(pc, None, perm, nr, mn)[0]
    res["shot_hist_us"] = device_us(lambda: ops.shot_hist(pc, None, perm, shot_normals, kp, kp_count, lrf, r), args.reps)[0]
    res["image_members_per_s"] = float(kpm.double().sum()) / (res["image_us"] * 1e-6)
    res["share_of_f64_vector_peak"] = None                               # no published or measured rate to hold it against

    if not args.skip_host:
        res["host_threads"] = args.threads
        k, kc = kp.cpu().numpy(), kp_count.cpu().numpy()
        hn = None
        res["host_normals_all_pairs_ms"] = 0.0
        if s > 0.0:
            t0 = time.perf_counter()
            hn = baselines.harris_normals_cpu(clouds, None, nr, mn, args.threads)[0]
            res["host_normals_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        hl, hlm = baselines.shot_frames_cpu(clouds, k, None, kc, r, args.threads)
        res["host_lrf_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        ha = np.ascontiguousarray(hl[:, :, 6:9])
        t0 = time.perf_counter()
        hh, hs, hk = baselines.spin_image_cpu(clouds, None, hn, k, kc, ha, r, s, st, args.threads)
        res["host_image_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_all_pairs_ms"] = sum(res["host_%s_all_pairs_ms" % x] for x in ("normals", "lrf", "image"))
        res["axes_equal_host_bits"] = bool(np.array_equal(axes.cpu().numpy().view(np.int64), ha.view(np.int64)))
        res["hist_equals_host"] = bool(np.array_equal(hist.cpu().numpy(), hh) and np.array_equal(kpm.cpu().numpy(), hk))
        res["spin_equals_host_bits"] = bool(np.array_equal(spin.cpu().numpy().view(np.int64), hs.view(np.int64)))
        res["device_over_host"] = res["descriptor_wall_ms"] / res["host_all_pairs_ms"]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
