#!/usr/bin/env python
"""gt.log and gt.info of fragment scenes, the files the indoor benchmark scores against
(evaluation/matlab/eval_indoor/3dmatch/getGtInfoLog.m), from the fragments' clouds and poses, on the device.

    python examples/make_fragment_ground_truth.py --scenes DIR --scene-names kitchen ... (--poses F44.npy | --info-dir DIR)
                                                  --out DIR
        reads <scenes>/<scene>/<i>.npy (rows x y z ...) and the fragments' camera-to-world poses -- either one array
        [F,4,4] (`{scene}` in the path is replaced by the scene's name) or <info-dir>/<scene>-info/cloud_bin_<i>.info.txt as
        depth-fusion writes them -- and writes <out>/<scene>-evaluation/gt.log and gt.info.
    python examples/make_fragment_ground_truth.py --make-synthetic DIR [--fragments 6] [--points 20000]
        writes a synthetic scene in examples/evaluate_fragments.py's layout (DIR/scenes/synthetic/<i>.npy,
        DIR/results/synthetic/<i>.bin) with DIR/info/synthetic-info/cloud_bin_<i>.info.txt, makes
        DIR/gt/synthetic-evaluation/gt.log and gt.info from the pose files, and scores the scene's landmark descriptors
        against them, as `examples/evaluate_fragments.py --scenes DIR/scenes --results DIR/results --gt DIR/gt
        --scene-names synthetic --dim D` does.

--leaf L (default 0.01, the reference's; 0: the clouds as they are), --far 0.03, --near 0.006, --cap 5000, --min-ratio 0.3,
--seed S (keys the thinning to 5000 correspondences).  Prints ONE JSON line."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usip_amd import fragments as fr            # noqa: E402
from usip_amd import ground_truth as gtm        # noqa: E402


def make_synthetic(root, fragments, points, dim, seed):
    sc = fr.synthetic_scene(seed, fragments, points, dim, ground_truth=False)
    scene, results, info = (os.path.join(root, "scenes", "synthetic"), os.path.join(root, "results", "synthetic"),
                            os.path.join(root, "info", "synthetic-info"))
    for d in (scene, results, info):
        os.makedirs(d, exist_ok=True)
    for i, cloud in enumerate(sc["clouds"]):
        np.save(os.path.join(scene, "%d.npy" % i), cloud)
        fr.write_descriptors_bin(os.path.join(results, "%d.bin" % i), sc["xyz"][i], sc["desc"][i])
        gtm.write_fragment_pose(os.path.join(info, "cloud_bin_%d.info.txt" % i), sc["poses"][i], "synthetic", i, i)
    return os.path.join(root, "scenes"), os.path.join(root, "results"), os.path.join(root, "info"), os.path.join(root, "gt")


def scene_clouds(scenes, name):
    paths = sorted(glob.glob(os.path.join(scenes, name, "*.npy")), key=lambda p: int(os.path.basename(p)[:-4]))
    if not paths:
        raise SystemExit("no fragments under %s" % os.path.join(scenes, name))
    return [np.load(p) for p in paths]


def scene_poses(name, count, args, info_dir):
    if info_dir:
        return np.stack([gtm.read_fragment_pose(os.path.join(info_dir, "%s-info" % name, "cloud_bin_%d.info.txt" % i))
                         for i in range(count)])
    poses = np.load(args.poses.replace("{scene}", name))
    if poses.shape != (count, 4, 4):
        raise SystemExit("%s holds %s, the scene has %d fragments" % (args.poses, poses.shape, count))
    return poses


def make_scene(name, scenes, info_dir, out, args):
    clouds = scene_clouds(scenes, name)
    poses = scene_poses(name, len(clouds), args, info_dir)
    start = time.time()
    gt, gt_info, pp = gtm.scene_ground_truth(clouds, poses, args.device, leaf=args.leaf or None, far=args.far, near=args.near,
                                             cap=args.cap, min_ratio=args.min_ratio, seed=args.seed,
                                             batch_pairs=args.batch_pairs)
    seconds = time.time() - start                                     # (ends in the scene's one host read)
    log, info = gtm.write_scene_ground_truth(os.path.join(out, "%s-evaluation" % name), gt, gt_info)
    return {"fragments": len(clouds), "pairs": int(len(pp["frag1"])), "written": len(gt), "seconds": seconds, "gt_log": log,
            "gt_info": info, "correspondences_mean": float(np.minimum(pp["hits"][pp["kept"], 1], args.cap).mean()) if len(gt)
            else 0.0}


def score_synthetic(scenes, results, gt_root, args):
    """examples/evaluate_fragments.py's evaluation of the scene, against the files just written."""
    clouds = scene_clouds(scenes, "synthetic")
    rows = [fr.read_descriptors_bin(os.path.join(results, "synthetic", "%d.bin" % i), args.dim) for i in range(len(clouds))]
    ev = fr.FragmentEvaluator(None, None, None, args.device, top=max(len(x) for x, _ in rows), seed=args.seed)
    for i, cloud in enumerate(clouds):
        ev.add_fragment_result(i, rows[i][0], rows[i][1], cloud)
    gt = fr.read_log(os.path.join(gt_root, "synthetic-evaluation", "gt.log"))
    gt_info = fr.read_info(os.path.join(gt_root, "synthetic-evaluation", "gt.info"))
    out = ev.evaluate(None, gt, gt_info)
    return {k: out[k] for k in ("pairs", "written", "recall", "precision", "good", "bad", "false_pos", "gt_num", "rs_num")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--make-synthetic", metavar="DIR")
    ap.add_argument("--fragments", type=int, default=6)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--scenes")
    ap.add_argument("--scene-names", nargs="+", default=[])
    ap.add_argument("--poses")
    ap.add_argument("--info-dir")
    ap.add_argument("--out")
    ap.add_argument("--leaf", type=float, default=gtm.LEAF)
    ap.add_argument("--far", type=float, default=gtm.FAR)
    ap.add_argument("--near", type=float, default=gtm.NEAR)
    ap.add_argument("--cap", type=int, default=gtm.CAP)
    ap.add_argument("--min-ratio", type=float, default=gtm.MIN_RATIO)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-pairs", type=int, default=None)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    out = {"leaf": args.leaf, "far": args.far, "near": args.near, "cap": args.cap, "min_ratio": args.min_ratio, "seed": args.seed}
    if args.make_synthetic:
        scenes, results, info_dir, gt_root = make_synthetic(args.make_synthetic, args.fragments, args.points, args.dim, args.seed)
        out["scenes"] = {"synthetic": make_scene("synthetic", scenes, info_dir, gt_root, args)}
        out["evaluation"] = score_synthetic(scenes, results, gt_root, args)
    elif args.scenes and args.scene_names and args.out and bool(args.poses) != bool(args.info_dir):
        out["scenes"] = {n: make_scene(n, args.scenes, args.info_dir, args.out, args) for n in args.scene_names}
    else:
        ap.error("give --make-synthetic DIR, or --scenes, --scene-names, --out and one of --poses and --info-dir")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
