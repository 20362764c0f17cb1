#!/usr/bin/env python
"""Train the descriptor on sequences of posed Nx8 .npy scans (x y z nx ny nz curvature reflectance) with 4x4 poses
(.npz with 'pose', as the reference's, or .npy), the batches built on the GPU (usip_amd.desc_pairs:
KittiDescriptorLoader semantics -- the positive a nearby scan of the same sequence, negatives mined from the poses) and
the keypoints taken from a frozen detector.  The checkpoint has the reference's keys (kitti/train_descriptor.py saves
model.descriptor.state_dict()) and loads into examples/evaluate_registration.py --descriptor_ckpt.

    python examples/train_descriptor_scans.py --make-synthetic /tmp/seqs                 # two synthetic sequences
    python examples/train_descriptor_scans.py --scans /data/00/np --poses /data/poses/00 \\
        --scans /data/01/np --poses /data/poses/01 --detector detector.pth --steps 1000
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_descriptor_scans.py --scans ...

One process per GPU; every rank holds the whole bank, takes its slice of each epoch's order (pair index rank * P + p)
and mines its negatives among its own P anchors; the next batch is prefetched on a side stream; gradients are
all-reduced.  Without --detector a short detector is trained first on the same scans (usip_amd.pairs, DetectorStep)."""
import argparse
import glob
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usip_amd import desc_pairs, pairs                       # noqa: E402
from usip_amd.networks import DetectorOptions                # noqa: E402
from usip_amd.step import DetectorStep                       # noqa: E402


def make_synthetic(d, sequences=2, scans=40, rows=20480, seed=0):
    """DIR/<seq>/scans/%06d.npy and DIR/<seq>/poses/%06d.npz: one synthetic scene per sequence, seen from a
    straight-ish trajectory at ~0.8 m spacing (desc_pairs.synthetic_sequences)."""
    for q, (clouds, poses) in desc_pairs.synthetic_sequences(sequences, scans, rows, 0.8, seed).items():
        for sub in ("scans", "poses"):
            os.makedirs(os.path.join(d, "%02d" % q, sub), exist_ok=True)
        for i, (c, p) in enumerate(zip(clouds, poses)):
            np.save(os.path.join(d, "%02d" % q, "scans", "%06d.npy" % i), c)
            np.savez(os.path.join(d, "%02d" % q, "poses", "%06d.npz" % i), pose=p)
    return [(os.path.join(d, "%02d" % q, "scans"), os.path.join(d, "%02d" % q, "poses")) for q in range(sequences)]


def schedule(num_scans, P, seed, rank, world, steps, first_step=0):
    """(scan ids, step) for `steps` steps: this rank's slices of the epochs' shuffled orders."""
    step, epoch = 0, 0
    while step < steps:
        batches = list(desc_pairs.epoch_batches(num_scans, P, seed, epoch, rank, world))
        if not batches:
            raise SystemExit("%d scans are fewer than one global batch of %d" % (num_scans, P * world))
        for ids in batches:
            if step == steps:
                return
            yield ids, first_step + step
            step += 1
        epoch += 1


def train_detector(files, opt, args, dev, rank, world):
    """A short detector run with the existing pieces (examples/train_detector_scans.py): its state dict."""
    recipe = pairs.PairRecipe.kitti(opt)
    bank = pairs.ScanBank.from_paths(files, dev, radius_threshold=recipe.radius_threshold)
    builder = pairs.PairBuilder(bank, recipe, args.pairs, dev, seed=args.seed, rank=rank)
    torch.manual_seed(0)
    st = DetectorStep(args.model, opt, dev, with_optimizer=True, graph=False)
    for it, batch in enumerate(builder.prefetch(schedule(bank.num_scans, args.pairs, args.seed, rank, world,
                                                         args.detector_steps))):
        loss = st.step(batch, epoch=None)
        if rank == 0 and (it % 10 == 0 or it == args.detector_steps - 1):
            print("detector step %4d  loss %.5f" % (it, float(loss.detach())), flush=True)
    return st.detector.state_dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", action="append", default=[], help="directory of one sequence's Nx8 .npy scans (repeatable)")
    ap.add_argument("--poses", action="append", default=[], help="directory of that sequence's poses (repeatable)")
    ap.add_argument("--make-synthetic", default=None, metavar="DIR", help="write synthetic sequences to DIR and use them")
    ap.add_argument("--synthetic-rows", type=int, default=20480)
    ap.add_argument("--synthetic-scans", type=int, default=40, help="scans per synthetic sequence (at least 40)")
    ap.add_argument("--detector", default=None, metavar="CKPT", help="detector checkpoint (otherwise one is trained)")
    ap.add_argument("--detector-steps", type=int, default=30)
    ap.add_argument("--model", default="ball", choices=["ball", "som"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--test-batches", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--cs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="descriptor.pth")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    dirs = list(zip(args.scans, args.poses))
    if len(args.scans) != len(args.poses):
        raise SystemExit("--scans and --poses come in pairs, one per sequence")
    if args.make_synthetic:
        if rank == 0:
            make_synthetic(args.make_synthetic, scans=max(40, args.synthetic_scans),
                           rows=max(args.synthetic_rows, args.n), seed=args.seed)
        if world > 1:
            dist.barrier()
        dirs = [(os.path.join(args.make_synthetic, q, "scans"), os.path.join(args.make_synthetic, q, "poses"))
                for q in sorted(os.listdir(args.make_synthetic))]
    if not dirs:
        raise SystemExit("give --scans DIR --poses DIR per sequence, or --make-synthetic DIR")
    sequences = {}
    for q, (sd, pd) in enumerate(dirs):
        sc = sorted(glob.glob(os.path.join(sd, "*.npy")))
        po = sorted(glob.glob(os.path.join(pd, "*.npz"))) or sorted(glob.glob(os.path.join(pd, "*.npy")))
        if not sc or len(sc) != len(po):
            raise SystemExit("%s has %d scans, %s has %d poses" % (sd, len(sc), pd, len(po)))
        sequences[q] = (sc, po)
    opt = DetectorOptions(surface_normal_len=args.cs, node_knn_k_1=16, lr=args.lr, input_pc_num=args.n, node_num=args.m)
    if args.detector:
        detector_state = torch.load(args.detector, map_location=dev)
    else:
        detector_state = train_detector([f for sc, _ in sequences.values() for f in sc], opt, args, dev, rank, world)
    recipe = desc_pairs.DescriptorPairRecipe.kitti(opt)
    bank = desc_pairs.PosedScanBank.from_sequences(sequences, dev, min_points=recipe.N)
    builder = desc_pairs.DescriptorPairBuilder(bank, recipe, args.pairs, dev, seed=args.seed, rank=rank)
    tester = desc_pairs.DescriptorPairBuilder(bank, recipe, args.pairs, dev, seed=args.seed + 1, rank=rank, mode="test")
    trainer = desc_pairs.DescriptorTrainer(builder, args.model, detector_state, opt, dev, seed=args.seed,
                                           graph=not args.no_graph and world == 1)
    for it, batch in enumerate(builder.prefetch(schedule(bank.num_scans, args.pairs, args.seed, rank, world, args.steps))):
        trainer.train_step(batch, epoch=None)
        if rank == 0 and (it % 10 == 0 or it == args.steps - 1):
            lv = float(trainer.last_loss.detach())
            print("step %4d  loss %.5f  active %.1f%%  neg_fail %d" % (
                it, lv, 100.0 * float(trainer.last_active.detach().mean()), int(trainer.neg_fail_total)), flush=True)
            if not np.isfinite(lv):
                raise SystemExit("loss is not finite")
    test_loss, test_active = trainer.test_pass(tester, schedule(bank.num_scans, args.pairs, args.seed + 1, rank, world,
                                                                 args.test_batches, first_step=1 << 20))
    if rank == 0:
        print("test  loss %.5f  active %.1f%%  neg_fail %d" % (test_loss, 100.0 * test_active, int(trainer.neg_fail_total)))
        if trainer.save_if_best(args.out, test_loss):
            print("saved", args.out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
