#!/usr/bin/env python
"""Registration recall / precision on scene fragments, the reference's indoor benchmark
(evaluation/matlab/eval_indoor/3dmatch: runFragmentRegistration.m, writeLog.m, evaluate.m), on the device.

    python examples/evaluate_fragments.py --make-synthetic DIR [--fragments 6] [--points 20000]
        builds a synthetic room of planes and boxes cut into overlapping posed fragments under DIR:
        DIR/scenes/synthetic/<i>.npy, DIR/gt/synthetic-evaluation/gt.log and gt.info (from the poses; gt.info over the
        points overlapping under the true pose) and DIR/results/synthetic/<i>.bin ([xyz, descriptor] rows; the descriptor
        of a keypoint is the one-hot id of its landmark, so overlapping fragments share the true correspondences), then
        evaluates it.
    python examples/evaluate_fragments.py --scenes DIR --results DIR --gt DIR [--scene-names livingroom1 ...]
        evaluates data laid out as the reference's scripts expect: <scenes>/<scene>/<i>.npy, <results>/<scene>/<i>.bin,
        <gt>/<scene>-evaluation/gt.log and gt.info.

--registration ransac (default: register2Fragments.m) or fgr (eval_indoor/fgr/register2FragmentsFGR.m: Fast Global
Registration on the mutual nearest descriptors, at most 1024 keypoints per fragment; --k and --trials are not used).

--refine icp adds writeLogReconputeAlign.m: both fragments voxel-averaged at 0.04 m, the estimate refined by trimmed
point-to-point ICP (pcregrigid's InlierRatio 0.3; --refine-iterations N, default 20; --refine-tolerance T R, default 0.01 m
0.009 rad), the share of moved points within 0.05 m recomputed and the log gated by `> 0.15` instead of `> 0.23`.  The log
holds the unrefined estimate, as the reference's does; --log-transform refined writes the refined pose instead.
--refine-metric plane refines under pcregrigid's 'pointToPlane' metric instead (default point): the downsampled fragments
get their 9-nearest normals, and every kept point is drawn towards the plane through its nearest point.

--optimize (needs --refine icp) adds split_txt_compute_G.m and the robust pose-graph optimisation behind it: the dense
information matrix of every pair under its refined pose, the log's pairs as a pose graph, the loop closures the graph does
not support pruned (--optimize-tau2 X, default 0.04; --optimize-fill gt|estimate: what stands in for an odometry pair the log
lacks, default gt; --optimize-transform edge|graph: what the refined log holds, default edge).  The JSON line then also
carries loop_recall, loop_precision, loops_in and loops_kept, and <scene>_odom.log/.info, <scene>_loop.log/.info and
<scene>_reg_refine_all.log are written beside <scene>.log.

--descriptor-method fpfh (default learned: the descriptors of the results files) describes the keypoints by Fast Point Feature
Histograms over the fragment clouds instead (usip_amd.baselines.FpfhDescriptor, 33 columns; --fpfh-radius, default 0.25 m,
--fpfh-normal-radius, default 0.125 m, --fpfh-normals estimated|supplied: supplied reads columns 4 .. 6 of the fragment
files).  The keypoints are the results files' (--method results) or, with --method iss | harris | sift | random, --top of them
from usip_amd.baselines with the outdoor defaults times --scale (default 0.05): then no results file, no network and no
checkpoint is read.  --write-descriptors DIR writes DIR/<scene>/<i>.bin rows [x y z d0 .. d32].  (On the synthetic room the
results files' keypoints are shared landmarks and FPFH registers most pairs; a baseline detector's keypoints there are mostly
the random points that pad the count, which no two fragments share, so that run only shows that the path works.)
--descriptor-method shot does the same with SHOT-352 (usip_amd.baselines.ShotDescriptor, 352 columns; --shot-radius, default
0.25 m, --shot-normal-radius, default 0.125 m; --fpfh-normals chooses its normals too).
--descriptor-method spin does the same with spin images (usip_amd.baselines.SpinDescriptor, 153 columns; --spin-radius, default
0.25 m, --spin-axis-radius, default 0.25 m: the SHOT frame whose z is the axis, --spin-support-angle-cos, default 0: no support
angle and no normals, otherwise normals over 0.125 m or, with --fpfh-normals supplied, the files'; --spin-structure rectangular |
radial): the `spin` of evaluate.m's descriptorName comment.

--method tsf runs the reference's own pipeline (the `tsf` branch of evaluation/save_keypoints.py:262-351 behind its loaders,
evaluation/redwood_loader.py and data/match3d_eval_loader.py) on the fragment files alone: --input-pc-num rows of every
fragment, half of them FPS candidates, --node-num nodes (usip_amd.fragment_batch, built on the device in batches of
--describe-batch), the eval-mode detector (--detector-model ball | som, --detector-ckpt F), sigma-ordered NMS over --nms-radius
and the --top smallest sigmas, then the eval-mode descriptor (--descriptor-head global | plain, --descriptor-ckpt F; --dim is
its length).  Without a checkpoint the module is a seeded, untrained one (a plumbing run) and the JSON line says so.  Fragment
files with only x y z columns get normals and curvature on the device (9 neighbours, viewpoint at the origin).  No results file
is read.  --write-keypoints DIR writes DIR/<scene>/<i>.bin, the float32 [count, 3] files eval_rep.m reads.
--method results --descriptor-ckpt F describes the results files' keypoints by that checkpoint's descriptor instead of taking
the files' descriptors.

Prints ONE JSON line (what evaluate.m prints, per scene and as means, and the registrator) and writes <results>/<scene>.log as writeLog.m does;
with --pair-files also the i-j.rt.txt of every pair, as clusterCallback.m does."""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usip_amd import fragments as fr            # noqa: E402
from usip_amd import posegraph as pg            # noqa: E402

LOOP_KEYS = ("loop_recall", "loop_precision", "loops_in", "loops_kept")
SPIN_NORMAL_RADIUS = 0.125                      # metres: the normals a spin image's support angle reads, when one is set


def make_synthetic(root, fragments, points, dim, seed):
    sc = fr.synthetic_scene(seed, fragments, points, dim)
    scene, results, gt = (os.path.join(root, "scenes", "synthetic"), os.path.join(root, "results", "synthetic"),
                          os.path.join(root, "gt", "synthetic-evaluation"))
    for d in (scene, results, gt):
        os.makedirs(d, exist_ok=True)
    for i, cloud in enumerate(sc["clouds"]):
        np.save(os.path.join(scene, "%d.npy" % i), cloud)
        fr.write_descriptors_bin(os.path.join(results, "%d.bin" % i), sc["xyz"][i], sc["desc"][i])
    fr.write_log(os.path.join(gt, "gt.log"), sc["gt"])
    fr.write_info(os.path.join(gt, "gt.info"), sc["gt_info"])
    return os.path.join(root, "scenes"), os.path.join(root, "results"), os.path.join(root, "gt")


def add_fpfh_fragment(ev, i, xyz, cloud, args):
    """--descriptor-method fpfh | shot | spin: fragment i's keypoints -- the results file's (xyz [M,3]) or, with --method iss | harris |
    sift | random, --top of them from usip_amd.baselines at the outdoor defaults times --scale -- described by Fast Point Feature
    Histograms, by SHOT-352 or by spin images, over the fragment's cloud.  No network, no checkpoint."""
    import torch
    from usip_amd import baselines as bl
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(cloud).T, dtype=np.float32)).to(args.device)
    pc = t[:3].unsqueeze(0).contiguous()
    s = args.scale
    if args.method == "results":
        kp = torch.from_numpy(np.ascontiguousarray(np.asarray(xyz, np.float32).T)).to(args.device).unsqueeze(0)
    else:
        if args.method == "random":
            kp, count = bl.random_keypoints(pc, None, args.top, args.seed, [i])
        else:
            detect = {"iss": lambda: bl.IssDetector(num=args.top, seed=args.seed, salient_radius=2.0 * s, non_max_radius=2.0 * s),
                      "harris": lambda: bl.HarrisDetector(num=args.top, seed=args.seed, radius=1.0 * s),
                      "sift": lambda: bl.SiftDetector(num=args.top, seed=args.seed, min_scale=0.5 * s)}[args.method]()
            kp, count = detect(pc, None, [i])
        kp = kp[:, :, :int(count[0])]
    normals = None
    if args.fpfh_normals == "supplied":
        if t.shape[0] < 6:
            raise SystemExit("--fpfh-normals supplied: fragment %d has no normal columns (expected rows [x y z nx ny nz ..])" % i)
        normals = t[3:6].unsqueeze(0).contiguous()
    describe = bl.ShotDescriptor(args.shot_radius, args.shot_normal_radius) if args.descriptor_method == "shot" else \
        bl.SpinDescriptor(args.spin_radius, args.spin_axis_radius, args.spin_support_angle_cos, SPIN_NORMAL_RADIUS,
                          structure=args.spin_structure) if args.descriptor_method == "spin" else \
        bl.FpfhDescriptor(args.fpfh_radius, args.fpfh_normal_radius)
    desc = describe(pc, kp.contiguous(), None, None, normals)
    return ev.add_fragment_result(i, kp[0].t(), desc[0].t(), cloud)


def make_networks(args):
    """--method tsf, or --descriptor-ckpt: (detector or None, descriptor, what the JSON line says of them).  A module without a
    checkpoint is seeded and untrained, as examples/train_descriptor_indoor.py's detector is."""
    import torch
    from usip_amd import inference
    from usip_amd.networks import (DescriptorLiteOld, DescriptorLiteOldGlobal, IndoorDetectorOptions, IndoorOptions,
                                   build_detector)
    said, detector = {}, None
    if args.method == "tsf":
        torch.manual_seed(args.seed)
        detector = build_detector(args.detector_model, IndoorDetectorOptions(input_pc_num=args.input_pc_num,
                                                                             node_num=args.node_num)).to(args.device)
        if args.detector_ckpt:
            inference.load_detector_state(detector, torch.load(args.detector_ckpt, map_location="cpu"))
        said["detector"] = dict(model=args.detector_model, checkpoint=args.detector_ckpt or "untrained (seeded)")
    torch.manual_seed(args.seed + 1)
    head = DescriptorLiteOldGlobal if args.descriptor_head == "global" else DescriptorLiteOld
    descriptor = head(IndoorOptions(input_pc_num=args.input_pc_num, node_num=args.node_num,
                                    descriptor_len=args.dim)).to(args.device)
    if args.descriptor_ckpt:
        inference.load_detector_state(descriptor, torch.load(args.descriptor_ckpt, map_location="cpu"))
    said["descriptor"] = dict(head=args.descriptor_head, checkpoint=args.descriptor_ckpt or "untrained (seeded)")
    return detector, descriptor, said


def add_described_scene(ev, name, scenes, rows, args):
    """--method tsf: every fragment of the scene through usip_amd.fragment_batch.FragmentDescriber in batches; with rows (the
    results files' [xyz, descriptor]) their keypoints are described instead of the detector's."""
    import torch
    from usip_amd import fragment_batch as fb
    from usip_amd.networks import IndoorDetectorOptions
    bank = fb.FragmentScanBank.from_scene_dir(os.path.join(scenes, name), args.device)
    recipe = fb.FragmentBatchRecipe.match3d(IndoorDetectorOptions(input_pc_num=args.input_pc_num, node_num=args.node_num))
    detector, descriptor, said = make_networks(args)
    describer = fb.FragmentDescriber(detector, descriptor, fb.FragmentBatchBuilder(bank, recipe, seed=args.seed),
                                     nms_radius=args.nms_radius, top=ev.top)
    for base in range(0, bank.num_scans, args.describe_batch):
        ids = list(range(base, min(base + args.describe_batch, bank.num_scans)))
        if rows is None:
            out = describer.describe(ids)
        else:
            kp = np.zeros((len(ids), 3, ev.top), np.float32)
            for b, i in enumerate(ids):                       # padded with the fragment's first keypoint, as the detector's are
                x = np.asarray(rows[i][0], np.float32).T
                kp[b] = x[:, :1]
                kp[b, :, :x.shape[1]] = x
            count = torch.tensor([len(rows[i][0]) for i in ids], dtype=torch.int32)
            out = describer.describe_keypoints(ids, torch.from_numpy(kp), count)
        ev.add_described(ids, out["kp"], out["desc"], out["count"], [bank.xyz(i) for i in ids])
        if args.write_keypoints:
            fb.write_keypoints_dir(os.path.join(args.write_keypoints, name), ids, out["kp"], out["count"])
    return said


def evaluate_scene(name, scenes, results, gt_root, args):
    if args.method == "tsf":                                    # <i>.npy or cloud_bin_<i>.npy: usip_amd.fragment_batch reads them
        clouds = glob.glob(os.path.join(scenes, name, "*.npy"))
    else:
        clouds = sorted(glob.glob(os.path.join(scenes, name, "*.npy")), key=lambda p: int(os.path.basename(p)[:-4]))
    if not clouds:
        raise SystemExit("no fragments under %s" % os.path.join(scenes, name))
    rows = None
    if args.method == "results":
        rows = [fr.read_descriptors_bin(os.path.join(results, name, "%d.bin" % i), args.dim) for i in range(len(clouds))]
    top = max(len(x) for x, _ in rows) if rows is not None else args.top
    ev = fr.FragmentEvaluator(None, None, None, args.device, top=top, k=args.k, max_trials=args.trials, seed=args.seed,
                              batch_pairs=args.batch_pairs, registrator=args.registration, refine=args.refine == "icp",
                              refine_args=dict(max_iterations=args.refine_iterations, tolerance=tuple(args.refine_tolerance)),
                              refine_metric={"point": "point_to_point", "plane": "point_to_plane"}[args.refine_metric],
                              log_transform=args.log_transform, optimize=args.optimize,
                              optimize_args=dict(tau2=args.optimize_tau2, fill=args.optimize_fill,
                                                 transform=args.optimize_transform) if args.optimize else None)
    said = None
    if args.method == "tsf" or args.descriptor_ckpt:
        said = add_described_scene(ev, name, scenes, rows, args)
    for i, path in enumerate(clouds if said is None else ()):
        if args.descriptor_method != "learned":
            add_fpfh_fragment(ev, i, rows[i][0] if rows is not None else None, np.load(path), args)
        else:
            ev.add_fragment_result(i, rows[i][0], rows[i][1], np.load(path))
    if args.write_descriptors:
        os.makedirs(os.path.join(args.write_descriptors, name), exist_ok=True)
        for i in ev.ids():
            fr.write_descriptors_bin(os.path.join(args.write_descriptors, name, "%d.bin" % i), *ev.fragment_arrays(i))
    gt = fr.read_log(os.path.join(gt_root, "%s-evaluation" % name, "gt.log"))
    gt_info = fr.read_info(os.path.join(gt_root, "%s-evaluation" % name, "gt.info"))
    out = ev.evaluate(None, gt, gt_info)
    fr.write_result_log(os.path.join(results, "%s.log" % name), out["entries"])
    if args.pair_files:
        pp, ids = out["per_pair"], ev.ids()
        os.makedirs(os.path.join(results, name, "registration-results"), exist_ok=True)
        for p in range(out["pairs"]):
            a, b = ids[pp["frag1"][p]], ids[pp["frag2"][p]]
            fr.write_pair_file(os.path.join(results, name, "registration-results", "%d-%d.rt.txt" % (a, b)),
                               fr.PairFile(a, b, int(pp["inliers"][p]), float(pp["inlier_ratio"][p]),
                                           tuple(pp["ratio_aligned"][p]), fr.to4x4(pp["Rt"][p]), pp["information"][p]))
    if args.optimize:
        pg.write_split(results, name, *out["split"])
        pg.write_refined(results, name, out["refined_entries"])
    scene = {k: out[k] for k in ("pairs", "written", "recall", "precision", "inlier_num_mean", "inlier_ratio_mean", "good",
                                  "bad", "false_pos", "gt_num", "rs_num") + (LOOP_KEYS if args.optimize else ())}
    if said is not None:
        scene["networks"] = said
    return scene


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--make-synthetic", metavar="DIR")
    ap.add_argument("--fragments", type=int, default=6)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--scenes")
    ap.add_argument("--results")
    ap.add_argument("--gt")
    ap.add_argument("--scene-names", nargs="+", default=["livingroom1", "livingroom2", "office1", "office2"])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=fr.K_MATCH)
    ap.add_argument("--trials", type=int, default=fr.MAX_TRIALS)
    ap.add_argument("--registration", choices=("ransac", "fgr"), default="ransac")
    ap.add_argument("--refine", choices=("none", "icp"), default="none")
    ap.add_argument("--refine-metric", choices=("point", "plane"), default="point")
    ap.add_argument("--log-transform", choices=("estimate", "refined"), default="estimate")
    ap.add_argument("--refine-tolerance", type=float, nargs=2, metavar=("T", "R"), default=list(fr.REFINE_TOLERANCE))
    ap.add_argument("--refine-iterations", type=int, default=fr.REFINE_ITERATIONS)
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--optimize-tau2", type=float, default=pg.TAU2)
    ap.add_argument("--optimize-fill", choices=("gt", "estimate"), default="gt")
    ap.add_argument("--optimize-transform", choices=("edge", "graph"), default="edge")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-pairs", type=int, default=32)
    ap.add_argument("--pair-files", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--descriptor-method", choices=("learned", "fpfh", "shot", "spin"), default="learned")
    ap.add_argument("--method", choices=("results", "iss", "harris", "sift", "random", "tsf"), default="results")
    ap.add_argument("--detector-ckpt", metavar="F")
    ap.add_argument("--detector-model", choices=("ball", "som"), default="ball")
    ap.add_argument("--descriptor-ckpt", metavar="F")
    ap.add_argument("--descriptor-head", choices=("global", "plain"), default="global")
    ap.add_argument("--input-pc-num", type=int, default=10240)
    ap.add_argument("--node-num", type=int, default=512)
    ap.add_argument("--nms-radius", type=float, default=0.1)
    ap.add_argument("--describe-batch", type=int, default=8)
    ap.add_argument("--write-keypoints", metavar="DIR")
    ap.add_argument("--top", type=int, default=512)
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--fpfh-radius", type=float, default=0.25)
    ap.add_argument("--fpfh-normal-radius", type=float, default=0.125)
    ap.add_argument("--fpfh-normals", choices=("estimated", "supplied"), default="estimated")
    ap.add_argument("--shot-radius", type=float, default=0.25)
    ap.add_argument("--shot-normal-radius", type=float, default=0.125)
    ap.add_argument("--spin-radius", type=float, default=0.25)
    ap.add_argument("--spin-axis-radius", type=float, default=0.25)
    ap.add_argument("--spin-support-angle-cos", type=float, default=0.0)
    ap.add_argument("--spin-structure", choices=("rectangular", "radial"), default="rectangular")
    ap.add_argument("--write-descriptors", metavar="DIR")
    args = ap.parse_args()
    if args.method == "tsf" and args.descriptor_method != "learned":
        ap.error("--method tsf describes by the learned descriptor (--descriptor-ckpt), not --descriptor-method %s"
                 % args.descriptor_method)
    if args.detector_ckpt and args.method != "tsf":
        ap.error("--detector-ckpt needs --method tsf")
    if args.descriptor_ckpt and (args.method not in ("tsf", "results") or args.descriptor_method != "learned"):
        ap.error("--descriptor-ckpt needs --method tsf or --method results, and --descriptor-method learned")
    if args.write_keypoints and args.method != "tsf":
        ap.error("--write-keypoints needs --method tsf")
    for ckpt in (args.detector_ckpt, args.descriptor_ckpt):
        if ckpt and not os.path.isfile(ckpt):
            ap.error("no checkpoint at %s" % ckpt)
    if args.describe_batch < 1 or args.input_pc_num < 2 or not 1 <= args.node_num <= args.input_pc_num // 2:
        ap.error("--describe-batch >= 1, --input-pc-num >= 2 and 1 <= --node-num <= --input-pc-num / 2")
    if args.method not in ("results", "tsf") and args.descriptor_method == "learned":
        ap.error("--method %s needs --descriptor-method fpfh, shot or spin (the results files hold the learned descriptors)"
                 % args.method)
    if args.log_transform == "refined" and args.refine != "icp":
        ap.error("--log-transform refined needs --refine icp")
    if args.optimize and args.refine != "icp":
        ap.error("--optimize needs --refine icp")
    if args.refine_metric != "point" and args.refine != "icp":
        ap.error("--refine-metric plane needs --refine icp")
    if args.make_synthetic:
        scenes, results, gt = make_synthetic(args.make_synthetic, args.fragments, args.points, args.dim, args.seed)
        names = ["synthetic"]
    elif args.scenes and args.results and args.gt:
        scenes, results, gt, names = args.scenes, args.results, args.gt, args.scene_names
    else:
        ap.error("give --make-synthetic DIR, or --scenes, --results and --gt")
    per_scene = {n: evaluate_scene(n, scenes, results, gt, args) for n in names}
    out = {"scenes": per_scene, "registration": args.registration}
    if args.descriptor_method != "learned" or args.method == "tsf":
        out.update(descriptor_method=args.descriptor_method, method=args.method)
    if args.refine != "none":
        out.update(refine=args.refine, log_transform=args.log_transform)
    if args.refine_metric != "point":
        out.update(refine_metric=args.refine_metric)
    for k in ("recall", "precision", "inlier_num_mean", "inlier_ratio_mean"):          # evaluate.m's last line: means
        out[k] = float(np.mean([s[k] for s in per_scene.values()]))
    for k in ("pairs", "written"):
        out[k] = int(sum(s[k] for s in per_scene.values()))
    if args.optimize:
        out["optimize"] = dict(tau2=args.optimize_tau2, fill=args.optimize_fill, transform=args.optimize_transform)
        for k in LOOP_KEYS[:2]:
            out[k] = float(np.mean([s[k] for s in per_scene.values()]))
        for k in LOOP_KEYS[2:]:
            out[k] = int(sum(s[k] for s in per_scene.values()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
