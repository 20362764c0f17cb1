#!/usr/bin/env python
"""Times of the f-17 SIFT3D baseline detector (usip_amd/baselines.py) at tools/iss_bench.py's shape: B = 8 frames of N = 16384
points, usip_amd.synth slab clouds, the reference's parameters (min_scale 0.5, 4 octaves, 8 scales per octave, min_contrast
0.1, field z), 512 keypoints per frame.  Per octave the device time of (a) the voxel average (keys, the sort of the keys, the
average), (b) the sort along x, (c) the scale space, (d) the 25 nearest, (e) the extrema; then (f) the selection; the share of
tile pairs the scale-space workgroups walk (from the counts the kernel writes) and the rows of every octave cloud; the library's
host twin (all pairs) on `--threads` threads; and, in the same call on the same device, the whole ISS and Harris3D detectors at
their own defaults.  ONE JSON line, also written to --out.

    python tools/sift_bench.py [--reps 10] [--threads 16] [--skip-host] [--out profiles/f17_sift_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f17_sift_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sift_bench needs a GPU"
    B, N = args.frames, args.points
    rng = np.random.default_rng(11)                                    # (tools/iss_bench.py's clouds)
    clouds = np.stack([synth.make_cloud(rng, N, "slab") for _ in range(B)]).astype(np.float32)
    pc = torch.from_numpy(clouds).cuda()
    P = dict(baselines.SIFT_DEFAULTS)
    k, contrast = P["n_scales_per_octave"], P["min_contrast"]
    res = {"metric": "f17_sift", "device": torch.cuda.get_device_name(0), "host": platform.node(), "frames": B, "points": N,
           "keypoints_per_frame": args.num, **P}

    tiles = (N + 255) // 256
    cloud, cnt = pc, None
    octaves, total_us = [], 0.0
    for o in range(P["n_octaves"]):
        base = P["min_scale"] * 2.0 ** o
        src, src_cnt, fld_arg = cloud, cnt, P["field"]                    # (an axis: each octave takes its own coordinate)
        cloud, fld, cnt = baselines.sift_octave(src, fld_arg, src_cnt, base)
        perm = baselines.sort_along_x(cloud, cnt)
        sigma2 = baselines.sift_sigma2(base, k)
        dog, visits = ops.sift_dog(cloud, fld, cnt, perm, sigma2, want_visits=True)
        idx = ops.sift_nearest(cloud, cnt, perm)
        mask, sidx = ops.sift_extrema(dog, idx, cnt, contrast)
        rows = cnt.tolist()
        live_tiles = sum(((r + 255) // 256) ** 2 for r in rows if r >= 25)
        oc = {"leaf": base, "walk_radius": baselines.sift_walk_radius(sigma2), "rows_per_frame": rows,
              "keypoints_per_frame": [int(v) for v in mask.sum(1).tolist()],
              "tile_pairs_walked": int(visits.sum()), "tile_pairs_of_the_live_rows": live_tiles,
              "tile_pairs_walked_share": (float(visits.sum()) / live_tiles) if live_tiles else None,
              "tile_pairs_walked_share_of_all_slots": float(visits.sum()) / (B * tiles * tiles)}
        stages = {"voxel_average_us": lambda: baselines.sift_octave(src, fld_arg, src_cnt, base),
                  "sort_x_us": lambda: baselines.sort_along_x(cloud, cnt),
                  "scale_space_us": lambda: ops.sift_dog(cloud, fld, cnt, perm, sigma2),
                  "nearest_us": lambda: ops.sift_nearest(cloud, cnt, perm),
                  "extrema_us": lambda: ops.sift_extrema(dog, idx, cnt, contrast)}
        for name, fn in stages.items():
            oc[name], oc[name + "_all"] = device_us(fn, args.reps)
        oc["device_stages_total_ms"] = sum(oc[s] for s in stages) * 1e-3
        total_us += sum(oc[s] for s in stages)
        octaves.append(oc)
    res["octaves"] = octaves
    cand, mask, scale, counts = baselines.sift_keypoints(pc, None, **P)
    u = baselines._draws(B, cand.shape[2] + N, 0, None).cuda()
    res["selection_us"], res["selection_us_all"] = device_us(
        lambda: baselines._select_candidates(pc, None, cand, mask, args.num, True, u), args.reps)
    res["device_stages_total_ms"] = (total_us + res["selection_us"]) * 1e-3
    res["sift_keypoints_per_frame"] = [int(v) for v in mask.sum(1).tolist()]
    det = baselines.SiftDetector(num=args.num, **P)
    res["detector_wall_ms"] = wall_ms(lambda: (det(pc), torch.cuda.synchronize()))
    res["share_of_f64_vector_peak"] = None                               # no published or measured rate to hold it against

    # ISS and Harris3D at their defaults, same clouds, same device, same call
    idet, hdet = baselines.IssDetector(num=args.num), baselines.HarrisDetector(num=args.num)
    res["iss_same_call"] = {**baselines.ISS_DEFAULTS, "detector_wall_ms": wall_ms(lambda: (idet(pc), torch.cuda.synchronize()))}
    res["harris_same_call"] = {**baselines.HARRIS_DEFAULTS,
                               "detector_wall_ms": wall_ms(lambda: (hdet(pc), torch.cuda.synchronize()))}

    if not args.skip_host:
        res["host_threads"] = args.threads
        t0 = time.perf_counter()
        h = baselines.sift_keypoints_cpu(clouds, None, num_threads=args.threads, **P)
        res["host_all_pairs_ms"] = (time.perf_counter() - t0) * 1e3
        res["candidates_equal_host_bits"] = bool(np.array_equal(cand.cpu().numpy().view(np.int32), h[0].view(np.int32)))
        res["keypoints_equal_host"] = bool(np.array_equal(mask.cpu().numpy(), h[1]))
        res["scales_equal_host_bits"] = bool(np.array_equal(scale.cpu().numpy().view(np.int64), h[2].view(np.int64)))
        res["octave_counts_equal_host"] = bool(np.array_equal(counts.cpu().numpy(), h[3]))
        res["device_over_host"] = res["detector_wall_ms"] / res["host_all_pairs_ms"]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
