#!/usr/bin/env python
"""Scores a detector + descriptor the way the reference's MATLAB does (evaluation/matlab/eval_repeatability/eval_rep.m,
eval_outdoor/kitti/evaluate_kitti.m), on the GPU: keypoint repeatability and RANSAC registration of scan pairs, printed
as ONE JSON line.

    python examples/evaluate_registration.py --make-synthetic /tmp/eval_data
    python examples/evaluate_registration.py --data /tmp/eval_data --detector det.pth --descriptor desc.pth \\
        --write-descriptors /tmp/descriptors
    python examples/evaluate_registration.py --data /tmp/eval_data --method iss      # or harris, sift, random: the baselines' numbers
    python examples/evaluate_registration.py --data /tmp/eval_data --method iss --descriptor-method fpfh   # no network at all

Data layout: <dir>/<id>.bin float32 rows [x y z nx ny nz curvature] and <dir>/pairs.txt with one pair per line,
`anc_id pos_id tx ty tz qw qx qy qz`: the pose that moves the positive scan into the anchor's frame.  Without checkpoints
the weights are the repository's seeded ones (usip_amd.synth.fill_parameters): the numbers then say nothing about USIP,
only that the pipeline runs.  --method iss | harris | sift | random scores the reference's baseline detectors (evaluation/save_keypoints.py)
instead of the learned one: --top keypoints per frame from usip_amd.baselines, described by the same descriptor.
--descriptor-method fpfh describes the keypoints by Fast Point Feature Histograms (usip_amd.baselines.FpfhDescriptor, 33 columns)
instead of the learned descriptor: with a baseline --method no network is constructed and no checkpoint is read.  --fpfh-normals
supplied takes the scans' own normals (columns 4 .. 6) instead of estimating them over --fpfh-normal-radius.
--descriptor-method shot does the same with SHOT-352 (usip_amd.baselines.ShotDescriptor, 352 columns; --shot-radius, default 2,
--shot-normal-radius, default 1): --method iss --top 256 --descriptor-method shot is the iss_256 + SHOT configuration the
reference's evaluate_kitti.m is set to.
--descriptor-method spin does the same with spin images (usip_amd.baselines.SpinDescriptor, 153 columns; --spin-radius, default
2, --spin-axis-radius, default the radius, --spin-support-angle-cos, default 0: no support angle, --spin-structure rectangular |
radial): the `spin` of eval_indoor/3dmatch/evaluate.m's descriptorName comment."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usip_amd import baselines, evaluation, inference, synth                       # noqa: E402
from usip_amd.networks import DescriptorLiteOld, DetectorOptions, build_detector   # noqa: E402

CS = 4


def quat_to_rot(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_synthetic(rng, frames: int, n: int):
    """-> (scans [(id, rows float32 [n, 3 + CS])], pairs [(anc_id, pos_id, T_gt 3x4)]): frame 0 is a slab-like scene with
    a few walls; every other frame is a rigidly moved, re-subsampled, jittered copy of it, paired with frame 0."""
    big = 2 * n
    pc = synth.make_cloud(rng, big, "slab:30").astype(np.float64)
    for k in range(12):                                       # walls: structure a detector can hold on to
        sel = slice(k * big // 24, (k + 1) * big // 24)
        pc[1, sel] = rng.uniform(-1, 4, sel.stop - sel.start)
        pc[0 if k % 2 else 2, sel] = rng.uniform(-30, 30)
    sn = synth.make_normals(rng, big, CS).astype(np.float64)
    scans, pairs = [], []
    for f in range(frames):
        pick = rng.permutation(big)[:n]
        if f == 0:
            R, t, q = np.eye(3), np.zeros(3), np.array([1.0, 0, 0, 0])
        else:
            yaw = rng.uniform(-0.3, 0.3)                      # about the vertical axis (y), plus a few metres
            q = np.array([np.cos(yaw / 2), 0, np.sin(yaw / 2), 0])
            R, t = quat_to_rot(q), rng.uniform(-3, 3, 3) * np.array([1, 0.1, 1])
        # the scan as seen from frame f: p_f = R' (p_0 - t), so that p_0 = R p_f + t
        pts = R.T @ (pc[:, pick] - t[:, None]) + rng.normal(0, 0.02, (3, n))
        nrm = np.concatenate((R.T @ sn[:3, pick], sn[3:, pick]))
        scans.append((f, np.ascontiguousarray(np.concatenate((pts, nrm)).T, dtype=np.float32)))
        if f:
            pairs.append((0, f, np.concatenate((R, t[:, None]), 1)))
    return scans, pairs


def write_dataset(folder, scans, pairs):
    os.makedirs(folder, exist_ok=True)
    for fid, rows in scans:
        rows.tofile(os.path.join(folder, "%06d.bin" % fid))
    with open(os.path.join(folder, "pairs.txt"), "w") as f:
        for a, q, T in pairs:
            R = T[:, :3]
            w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2          # small rotations: w is far from zero
            quat = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]
            f.write("%d %d %s\n" % (a, q, " ".join("%.17g" % v for v in list(T[:, 3]) + quat)))


def read_dataset(folder):
    pairs, ids = [], []
    for line in open(os.path.join(folder, "pairs.txt")):
        v = line.split()
        if not v:
            continue
        a, q, rest = int(v[0]), int(v[1]), [float(s) for s in v[2:11]]
        pairs.append((a, q, np.concatenate((quat_to_rot(rest[3:7]), np.asarray(rest[:3])[:, None]), 1)))
        ids += [a, q]
    scans = [(i, np.fromfile(os.path.join(folder, "%06d.bin" % i), dtype=np.float32).reshape(-1, 3 + CS))
             for i in sorted(set(ids))]
    return scans, pairs


def seeded(module):
    sd = module.state_dict()
    filled = synth.fill_parameters({k: tuple(v.shape) for k, v in sd.items()})
    module.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return module


def build_evaluator(model, detector_ckpt, top, nms_radius, max_trials, seed, descriptor_ckpt=None, device="cuda:0",
                    method="tsf", descriptor_method="learned"):
    dev = torch.device(device)
    opt = DetectorOptions(surface_normal_len=CS, node_knn_k_1=16)
    detector = build_detector(model, opt).to(dev) if method == "tsf" else None     # the baselines need none
    descriptor = DescriptorLiteOld(opt).to(dev) if descriptor_method == "learned" else None       # the hand-crafted ones need none
    if detector is None:
        pass
    elif detector_ckpt:
        inference.load_detector_state(detector, torch.load(detector_ckpt, map_location=dev))
    else:
        seeded(detector)
    if descriptor is None:
        pass
    elif descriptor_ckpt:
        inference.load_detector_state(descriptor, torch.load(descriptor_ckpt, map_location=dev))
    else:
        seeded(descriptor)
    return evaluation.RegistrationEvaluator(detector, descriptor, opt, dev, nms_radius=nms_radius, top=top,
                                            max_trials=max_trials, seed=seed)


def add_scans(evaluator, scans, nodes, seed, method="tsf", iss=None, harris=None, sift=None, fpfh=None, shot=None, spin=None):
    """method 'iss' / 'harris' / 'sift' / 'random': evaluator.top keypoints per frame from usip_amd.baselines (iss, harris,
    sift: IssDetector's / HarrisDetector's / SiftDetector's parameters; sift's field may be "x" | "y" | "z" or "curvature",
    the scans' seventh column).  fpfh: dict(radius, normal_radius, normals "estimated" | "supplied") -- the keypoints are
    described by baselines.FpfhDescriptor instead of the evaluator's descriptor.  shot: dict(radius, normal_radius) -- by
    baselines.ShotDescriptor.  spin: dict(radius, axis_radius, support_angle_cos, structure) -- by baselines.SpinDescriptor."""
    dev = evaluator.device
    fpfh = dict(fpfh) if fpfh is not None else None
    supplied = fpfh is not None and fpfh.pop("normals", "estimated") == "supplied"
    describe = baselines.FpfhDescriptor(**fpfh) if fpfh is not None else None
    if shot is not None:
        describe = baselines.ShotDescriptor(**shot)
    if spin is not None:
        describe = baselines.SpinDescriptor(**spin)

    def add(fid, pc, sn, kp, count):
        if describe is None:
            return evaluator.add_frame_keypoints(fid, pc, sn, kp, count)
        desc = describe(pc, kp, None, count, sn[:, :3].contiguous() if supplied else None)
        return evaluator.add_frame_descriptors(fid, kp, desc, count)

    detect = baselines.IssDetector(num=evaluator.top, seed=seed, **(iss or {})) if method == "iss" else \
        baselines.HarrisDetector(num=evaluator.top, seed=seed, **(harris or {})) if method == "harris" else None
    sift = dict(sift or {})
    curvature = sift.get("field") == "curvature"
    if method == "sift":
        detect = baselines.SiftDetector(num=evaluator.top, seed=seed, **dict(sift, field="z" if curvature else sift.get("field", "z")))
    for fid, rows in scans:
        t = torch.from_numpy(np.ascontiguousarray(rows.T)).to(dev)
        pc, sn = t[:3].unsqueeze(0).contiguous(), t[3:].unsqueeze(0).contiguous()
        if method == "tsf":
            first = torch.tensor([(seed + 7919 * int(fid)) % pc.shape[2]], dtype=torch.int32, device=dev)
            node = inference.sample_nodes(pc, nodes, first)
            if describe is None:
                evaluator.add_frame(fid, pc, sn, node)
            else:
                keypoints, sigmas = inference.run_model(evaluator.detector, pc, sn, node)
                add(fid, pc, sn, *evaluation.select_keypoints_device(keypoints, sigmas, evaluator.nms_radius, evaluator.top))
        else:
            if method == "sift" and curvature:
                kp, count = detect(pc, None, [int(fid)], field=t[6].unsqueeze(0).contiguous())
            else:
                kp, count = detect(pc, None, [int(fid)]) if detect is not None else \
                    baselines.random_keypoints(pc, None, evaluator.top, seed, [int(fid)])
            add(fid, pc, sn, kp, count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-synthetic", metavar="DIR", help="write a small synthetic dataset there and evaluate it")
    ap.add_argument("--data", metavar="DIR", help="evaluate the dataset in DIR")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--model", default="ball", choices=["ball", "som"])
    ap.add_argument("--detector", help="detector checkpoint (default: seeded weights)")
    ap.add_argument("--descriptor", help="descriptor checkpoint (default: seeded weights)")
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--top", type=int, default=256)
    ap.add_argument("--nms-radius", type=float, default=1.0)
    ap.add_argument("--max-trials", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--write-descriptors", metavar="DIR", help="write <id>.bin rows [x y z d0 .. d127] there (fpfh: d0 .. d32, shot: d0 .. d351, spin: d0 .. d152)")
    ap.add_argument("--method", default="tsf", choices=["tsf", "iss", "harris", "sift", "random"],
                    help="tsf: the learned detector; iss, harris, sift, random: the baselines, --top keypoints per frame")
    ap.add_argument("--salient-radius", type=float, default=2.0)
    ap.add_argument("--non-max-radius", type=float, default=2.0)
    ap.add_argument("--gamma-21", type=float, default=0.975)
    ap.add_argument("--gamma-32", type=float, default=0.975)
    ap.add_argument("--min-neighbors", type=int, default=5)
    ap.add_argument("--harris-radius", type=float, default=1.0)
    ap.add_argument("--harris-threshold", type=float, default=0.001)
    ap.add_argument("--sift-min-scale", type=float, default=0.5)
    ap.add_argument("--sift-octaves", type=int, default=4)
    ap.add_argument("--sift-scales", type=int, default=8)
    ap.add_argument("--sift-contrast", type=float, default=0.1)
    ap.add_argument("--sift-field", default="z", choices=["x", "y", "z", "curvature"])
    ap.add_argument("--descriptor-method", default="learned", choices=["learned", "fpfh", "shot", "spin"],
                    help="learned: the descriptor network (--descriptor is its checkpoint); fpfh: Fast Point Feature Histograms; "
                         "shot: SHOT-352; spin: spin images")
    ap.add_argument("--fpfh-radius", type=float, default=2.0)
    ap.add_argument("--fpfh-normal-radius", type=float, default=1.0)
    ap.add_argument("--fpfh-normals", default="estimated", choices=["estimated", "supplied"],
                    help="supplied: the scans' own normals (columns 4 .. 6) instead of estimated ones")
    ap.add_argument("--shot-radius", type=float, default=2.0)
    ap.add_argument("--shot-normal-radius", type=float, default=1.0)
    ap.add_argument("--spin-radius", type=float, default=2.0)
    ap.add_argument("--spin-axis-radius", type=float, default=None, help="the radius of the SHOT frame whose z is the axis "
                                                                         "(default: --spin-radius)")
    ap.add_argument("--spin-support-angle-cos", type=float, default=0.0,
                    help="> 0: only members whose estimated normal has |n . axis| at or above it")
    ap.add_argument("--spin-structure", default="rectangular", choices=["rectangular", "radial"])
    args = ap.parse_args()
    if args.make_synthetic:
        scans, pairs = make_synthetic(np.random.default_rng(args.seed), args.frames, args.points)
        write_dataset(args.make_synthetic, scans, pairs)
        args.data = args.make_synthetic
    if not args.data:
        ap.error("give --data DIR or --make-synthetic DIR")
    scans, pairs = read_dataset(args.data)
    evaluator = build_evaluator(args.model, args.detector, args.top, args.nms_radius, args.max_trials,
                                args.seed, args.descriptor, method=args.method, descriptor_method=args.descriptor_method)
    add_scans(evaluator, scans, args.nodes, args.seed, args.method,
              dict(salient_radius=args.salient_radius, non_max_radius=args.non_max_radius, gamma_21=args.gamma_21,
                   gamma_32=args.gamma_32, min_neighbors=args.min_neighbors),
              dict(radius=args.harris_radius, threshold=args.harris_threshold),
              dict(min_scale=args.sift_min_scale, n_octaves=args.sift_octaves, n_scales_per_octave=args.sift_scales,
                   min_contrast=args.sift_contrast, field=args.sift_field),
              dict(radius=args.fpfh_radius, normal_radius=args.fpfh_normal_radius, normals=args.fpfh_normals)
              if args.descriptor_method == "fpfh" else None,
              dict(radius=args.shot_radius, normal_radius=args.shot_normal_radius)
              if args.descriptor_method == "shot" else None,
              dict(radius=args.spin_radius, axis_radius=args.spin_axis_radius, support_angle_cos=args.spin_support_angle_cos,
                   structure=args.spin_structure)
              if args.descriptor_method == "spin" else None)
    summary = evaluator.evaluate(pairs)
    summary.pop("per_pair")
    fpfh = args.descriptor_method in ("fpfh", "shot", "spin")             # hand-crafted: there are no descriptor weights
    summary["seeded_weights"] = not ((args.detector or args.method != "tsf") and (args.descriptor or fpfh))
    summary["method"] = args.method
    if fpfh:                                                      # (the default's line is what it was)
        summary["descriptor_method"] = args.descriptor_method
    if args.write_descriptors:
        os.makedirs(args.write_descriptors, exist_ok=True)
        for fid, _ in scans:
            inference.write_descriptors_bin(os.path.join(args.write_descriptors, "%06d.bin" % fid),
                                            *evaluator.frame_arrays(fid))
    print(json.dumps({k: (None if isinstance(v, float) and v != v else v) for k, v in summary.items()}))   # NaN: no such pair


if __name__ == "__main__":
    main()
