#!/usr/bin/env python
"""Raw LiDAR scans -> the reference's Nx8 .npy scans (x y z nx ny nz curvature reflectance), prepared on the GPU
(usip_amd.prepare: nine nearest neighbours, normal and curvature, voxel grid average at 0.2 m) -- what the reference does
with MATLAB (evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108).  The output directory is what
examples/train_detector_scans.py --scans takes.

    python examples/prepare_scans.py --velodyne /data/kitti/sequences/00/velodyne --out /data/kitti/00/np_0.20_20480_r90_sn
    python examples/prepare_scans.py --make-synthetic /tmp/prepared          # ring-structured raw scans, prepared
    python examples/train_detector_scans.py --scans /tmp/prepared --steps 100

--test-bin also writes <name>.bin, float32 [m,6] xyz + normal, as kitti_test_prepare.m writes its test scans.  Prints one
JSON line."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usip_amd import prepare, synth                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--velodyne", default=None, metavar="DIR", help="directory of raw float32 [n,4] .bin scans")
    ap.add_argument("--out", default=None, metavar="DIR", help="where the [m,8] .npy scans go")
    ap.add_argument("--make-synthetic", default=None, metavar="DIR", help="prepare synthetic ring scans into DIR")
    ap.add_argument("--scans", type=int, default=8, help="number of synthetic scans (one per pair of the default batch)")
    ap.add_argument("--test-bin", action="store_true", help="also write xyz + normal float32 [m,6] .bin files")
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--leaf", type=float, default=0.2)
    ap.add_argument("--max-rows", type=int, default=None, help="the reference keeps 20480 rows per scan")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if (args.velodyne is None) == (args.make_synthetic is None):
        raise SystemExit("give --velodyne DIR --out DIR, or --make-synthetic DIR")
    if args.velodyne and not args.out:
        raise SystemExit("--velodyne needs --out DIR")
    assert torch.cuda.is_available(), "prepare_scans needs a GPU"
    if args.make_synthetic:
        out = args.make_synthetic
        raw = [("%06d" % i, synth.make_ring_scan(args.seed + i)) for i in range(args.scans)]
    else:
        out = args.out
        files = sorted(glob.glob(os.path.join(args.velodyne, "*.bin")))
        if not files:
            raise SystemExit("no .bin scans in %s" % args.velodyne)
        raw = ((os.path.splitext(os.path.basename(f))[0], prepare.load_velodyne_bin(f)) for f in files)
    os.makedirs(out, exist_ok=True)
    prep = prepare.ScanPreparer("cuda:0", k=args.k, leaf=args.leaf, max_rows=args.max_rows, seed=args.seed)
    count = points = rows_out = 0
    ms = []
    for i, (name, scan) in enumerate(raw):
        pts = torch.from_numpy(scan).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = prep(pts, scan_id=i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        np.save(os.path.join(out, name + ".npy"), rows.cpu().numpy())
        if args.test_bin:
            prepare.save_test_bin(os.path.join(out, name + ".bin"), rows)
        count, points, rows_out = count + 1, points + scan.shape[0], rows_out + rows.shape[0]
    # (the first call loads the code objects and warms the allocator: the median leaves it out)
    print(json.dumps({"metric": "prepare_scans", "scans": count, "points_in": points, "rows_out": rows_out,
                      "ms_per_scan": float(np.median(ms)), "ms_first_scan": ms[0], "out": out}))


if __name__ == "__main__":
    main()
