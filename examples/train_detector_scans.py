#!/usr/bin/env python
"""Train the detector on a directory of the reference's Nx8 .npy scans (x y z nx ny nz curvature reflectance), with
the training pairs built on the GPU (usip_amd.pairs: KittiLoader / OxfordLoader semantics) and the checkpoint saved
with the reference's keys (kitti/train_detector.py saves model.detector.state_dict()).

    python examples/train_detector_scans.py --make-synthetic /tmp/scans          # a few synthetic scans, then train
    python examples/train_detector_scans.py --scans /data/kitti/00/np_0.20_20480_r90_sn --steps 1000
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_detector_scans.py --scans DIR

One process per GPU; every rank holds the whole bank, takes its slice of each epoch's order (pair index
rank * P + p) and builds its P pairs with the next batch prefetched on a side stream; gradients are all-reduced."""
import argparse
import glob
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usip_amd import pairs, synth                            # noqa: E402
from usip_amd.networks import DetectorOptions                # noqa: E402
from usip_amd.step import DetectorStep                       # noqa: E402


def make_synthetic(d, count=12, rows=20480, min_rows=15360, seed=0):
    """Slab clouds with unit normals, curvature and reflectance: the reference's Nx8 layout, min_rows..rows rows each
    (KITTI: some shorter than N take the fix_idx layout; Oxford needs at least N)."""
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(min(min_rows, rows), rows + 1))
        scan = np.concatenate([synth.make_cloud(rng, n, "slab").T, synth.make_normals(rng, n, 5).T], 1)
        np.save(os.path.join(d, "%06d.npy" % i), scan.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", default=None, help="directory of Nx8 .npy scans")
    ap.add_argument("--make-synthetic", default=None, metavar="DIR", help="write synthetic scans to DIR and use them")
    ap.add_argument("--synthetic-rows", type=int, default=20480, help="rows of the largest synthetic scan")
    ap.add_argument("--dataset", default="kitti", choices=["kitti", "oxford"])
    ap.add_argument("--model", default="ball", choices=["ball", "som"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--cs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="detector_scans.pth")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    root = args.scans
    if args.make_synthetic:
        if rank == 0:
            rows = max(args.synthetic_rows, args.n)
            floor = args.n if args.dataset == "oxford" else (3 * rows) // 4     # Oxford: every scan >= N rows
            make_synthetic(args.make_synthetic, rows=rows, min_rows=floor)
        if world > 1:
            dist.barrier()
        root = args.make_synthetic
    files = sorted(glob.glob(os.path.join(root, "*.npy")))
    if not files:
        raise SystemExit("no .npy scans in %s" % root)
    opt = DetectorOptions(surface_normal_len=args.cs, node_knn_k_1=16, lr=args.lr, input_pc_num=args.n, node_num=args.m)
    recipe = pairs.PairRecipe.kitti(opt) if args.dataset == "kitti" else pairs.PairRecipe.oxford(opt)
    bank = pairs.ScanBank.from_paths(files, dev, radius_threshold=recipe.radius_threshold)
    builder = pairs.PairBuilder(bank, recipe, args.pairs, dev, seed=args.seed, rank=rank)
    torch.manual_seed(0)                                     # identical replicas on every rank
    st = DetectorStep(args.model, opt, dev, with_optimizer=True, graph=not args.no_graph and world == 1)

    def schedule():
        step, epoch = 0, 0
        while step < args.steps:
            batches = list(pairs.epoch_batches(bank.num_scans, args.pairs, args.seed, epoch, rank, world))
            if not batches:
                raise SystemExit("%d scans are fewer than one global batch of %d" % (bank.num_scans, args.pairs * world))
            for ids in batches:
                if step == args.steps:
                    return
                yield ids, step
                step += 1
            epoch += 1

    for it, batch in enumerate(builder.prefetch(schedule())):
        loss = st.step(batch, epoch=None)
        if rank == 0 and (it % 10 == 0 or it == args.steps - 1):
            lv = float(loss.detach())
            print("step %4d  loss %.5f  chamfer %.5f" % (it, lv, float(st.last["chamfer_pure"])), flush=True)
            if not np.isfinite(lv):
                raise SystemExit("loss is not finite")
    if rank == 0:
        torch.save(st.detector.state_dict(), args.out)
        print("saved", args.out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
