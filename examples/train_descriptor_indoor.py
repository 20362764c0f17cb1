#!/usr/bin/env python
"""Train the indoor descriptor (the head with the global context, models/networks.py:388-479, and the CGF triplet loss, as
ModelDescriptorIndoor.optimize strings them together) for a few steps on synthetic slab pairs, and save a checkpoint whose keys
are the reference's (scenenn/train_descriptor.py saves model.descriptor.state_dict()): conv1..conv5, fc1..fc3.

    python examples/train_descriptor_indoor.py --make-synthetic /tmp/indoor --steps 20

A pair is a slab cloud and the same cloud under a known rigid motion with jitter; keypoints are a subset of the points, so most
anchors have a positive within opt.CGF_radius.  Prints ONE JSON line.

On SceneNN-layout data (info_<mode>.pkl with pairs_np and icp_np, frames_<mode>/<i>.npy; usip_amd.indoor_pairs) the batches
are built on the GPU and a frozen detector gives the keypoints, as scenenn/train_descriptor.py does it:

    python examples/train_descriptor_indoor.py --make-synthetic-scenenn /tmp/scenenn --epochs 2
    python examples/train_descriptor_indoor.py --dataroot /data/scenenn --detector-ckpt detector/best.pth --epochs 500

--make-synthetic-scenenn writes a small dataset of that layout from slab scenes with known poses first, then trains on it;
without --detector-ckpt the detector is a seeded, untrained one (a plumbing run).  train + val are trained on, test is
tested on after every epoch, and the checkpoint is written by the reference's rule."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usip_amd import synth                                   # noqa: E402
from usip_amd.networks import IndoorOptions                  # noqa: E402
from usip_amd.step import IndoorDescriptorStep, batch_to_device   # noqa: E402


def scenenn(args, dev):
    """Train on <root>: train + val through one 'bank'-mode builder, a test pass per epoch, the reference's checkpoint rule."""
    from usip_amd import indoor_pairs
    from usip_amd.networks import build_detector
    root = args.dataroot or args.make_synthetic_scenenn
    made = None
    if args.make_synthetic_scenenn:
        made = indoor_pairs.synthetic_scenenn(root, frames=6, rows=max(args.n + args.n // 5, 600), seed=args.seed)
    opt = IndoorOptions(lr=args.lr, input_pc_num=args.n, node_num=args.m, batch_size=args.pairs)
    if args.detector_ckpt:
        state = torch.load(args.detector_ckpt, map_location="cpu")
    else:                                                    # a seeded, untrained detector: its sigmas are large
        torch.manual_seed(args.seed)
        state = build_detector("ball", opt).state_dict()
        opt.sigma_max = 5.0
    recipe = indoor_pairs.IndoorPairRecipe.scenenn(opt)
    train = indoor_pairs.IndoorPairBank.from_root(root, "train", dev) + indoor_pairs.IndoorPairBank.from_root(root, "val", dev)
    test = indoor_pairs.IndoorPairBank.from_root(root, "test", dev)
    builder = indoor_pairs.IndoorPairBuilder(train, recipe, args.pairs, dev, seed=args.seed, mode="bank")
    tester = indoor_pairs.IndoorPairBuilder(test, recipe, 1, dev, seed=args.seed + 1, mode="test")
    trainer = indoor_pairs.IndoorDescriptorTrainer(builder, "ball", state, opt, dev, seed=args.seed, graph=not args.no_graph,
                                                   min_save_epoch=0 if made else 8)
    out = os.path.join(root, "descriptor_indoor.pth")
    step, losses, active, written, test_loss, test_active = 0, [], [], False, None, None
    for epoch in range(args.epochs):
        schedule = [(ids, step + k) for k, ids in enumerate(
            indoor_pairs.epoch_batches(train.num_samples, args.pairs, args.seed, epoch))]
        step += len(schedule)
        batches = builder.prefetch(schedule) if args.prefetch else (builder.build(ids, s) for ids, s in schedule)
        epoch_losses = [(trainer.train_step(batch, epoch=epoch).detach().clone(), trainer.last_active.detach().clone())
                        for batch in batches]
        both = torch.stack([torch.stack((a, b)) for a, b in epoch_losses]).cpu()  # the epoch's one read-back
        losses += both[:, 0].tolist()
        active += both[:, 1].tolist()
        test_loss, test_active = trainer.test_pass(tester, [([i], i) for i in range(test.num_samples)])
        written = trainer.save_if_best(out, test_loss, epoch) or written
    keys = len(torch.load(out, map_location="cpu")) if written else 0
    print(json.dumps(dict(root=root, synthetic=made, epochs=args.epochs, steps=len(losses), pairs=args.pairs, n=args.n, m=args.m,
                          samples=dict(train_val=train.num_samples, test=test.num_samples), first_loss=losses[0],
                          train_loss=sum(losses) / len(losses), test_loss=test_loss, mean_active=sum(active) / len(active),
                          test_active=test_active, checkpoint_written=written, checkpoint=out if written else None,
                          keys=keys, prefetch=bool(args.prefetch))))


def main():
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--make-synthetic", metavar="DIR", help="synthetic slab pairs; where the checkpoint goes")
    mode.add_argument("--dataroot", metavar="DIR", help="SceneNN-layout data: info_<mode>.pkl and frames_<mode>/")
    mode.add_argument("--make-synthetic-scenenn", metavar="DIR", help="write a small dataset of that layout, train on it")
    ap.add_argument("--detector-ckpt", help="the frozen detector's state dict (--dataroot / --make-synthetic-scenenn)")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--prefetch", action="store_true", help="build batch k+1 on a side stream during step k")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.make_synthetic is None:
        return scenenn(args, dev)
    torch.manual_seed(args.seed)
    opt = IndoorOptions(lr=args.lr, input_pc_num=args.n, node_num=args.m, batch_size=args.pairs)
    st = IndoorDescriptorStep(opt, dev, with_optimizer=True, graph=not args.no_graph, seed=args.seed)
    losses, active = [], []
    for it in range(args.steps):
        batch = batch_to_device(synth.make_indoor_pair_batch(1000 * args.seed + it, args.pairs, args.n, args.m,
                                                             opt.surface_normal_len), dev)
        losses.append(float(st.step(batch).detach()))
        active.append(float(st.last["active_percentage"]))
    os.makedirs(args.make_synthetic, exist_ok=True)
    out = os.path.join(args.make_synthetic, "descriptor_indoor.pth")
    sd = {k: v.detach().cpu().clone() for k, v in st.descriptor.state_dict().items()}
    torch.save(sd, out)
    print(json.dumps(dict(steps=args.steps, pairs=args.pairs, n=args.n, m=args.m, first_loss=losses[0], last_loss=losses[-1],
                          mean_active=sum(active) / len(active), checkpoint=out, keys=len(sd),
                          layers=sorted({k.split(".")[0] for k in sd}))))


if __name__ == "__main__":
    main()
