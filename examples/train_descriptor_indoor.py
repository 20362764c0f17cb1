#!/usr/bin/env python
"""Train the indoor descriptor (the head with the global context, models/networks.py:388-479, and the CGF triplet loss, as
ModelDescriptorIndoor.optimize strings them together) for a few steps on synthetic slab pairs, and save a checkpoint whose keys
are the reference's (scenenn/train_descriptor.py saves model.descriptor.state_dict()): conv1..conv5, fc1..fc3.

    python examples/train_descriptor_indoor.py --make-synthetic /tmp/indoor --steps 20

A pair is a slab cloud and the same cloud under a known rigid motion with jitter; keypoints are a subset of the points, so most
anchors have a positive within opt.CGF_radius.  The SceneNN / 3DMatch loaders and their ICP pose files are not part of this
package: a real loader hands IndoorDescriptorStep.step the same ten tensors.  Prints ONE JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usip_amd import synth                                   # noqa: E402
from usip_amd.networks import IndoorOptions                  # noqa: E402
from usip_amd.step import IndoorDescriptorStep, batch_to_device   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-synthetic", metavar="DIR", required=True, help="where the checkpoint goes")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
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
