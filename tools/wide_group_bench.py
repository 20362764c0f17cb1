#!/usr/bin/env python
"""Times of the descriptor step at the indoor model's own shape (scenenn/options_descriptor.py: ball_nsamples 448, ball_radius
0.75, 5000 points, 512 keypoints, 2 pairs; descriptor_len 128): forward + backward + Adam of usip_amd.step.DescriptorStep on the
wide-group kernels (csrc/group_wide.hip) against ops.WIDE_GROUPS off -- the activated 128 x 917 504 tensor materialised and
pooled by group_max_kernel<64>, the literal cat(h, expand(pooled)) in front of conv4, the pooling gradient written dense -- in
ONE process, alternating.  Beside it the peak device memory of both forms above what the inputs and the model hold, and the two
new kernels stand-alone with the bytes they move.  ONE JSON line, also written to --out.  No ratio is asserted anywhere.

    python tools/wide_group_bench.py [--rounds 4] [--reps 5] [--precision f32x2] [--out profiles/f23_wide_group_bench.json]

Step times: events on the launch stream around `reps` back-to-back eager steps after a warm-up; `rounds` alternating rounds
(fused, fallback, fused, ...), the median of every round's windows listed per form.  `fused_below_fallback` says whether EVERY
fused median lies below EVERY fallback median on this box."""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from usip_amd import ops, synth                              # noqa: E402
from usip_amd.networks import DetectorOptions                # noqa: E402
from usip_amd.step import DescriptorStep, batch_to_device    # noqa: E402
from iss_bench import device_us                              # noqa: E402


def make_batch(pairs, n, kp, seed=23):
    """synthetic slab clouds of 6 m x 6 m (a fragment's extent): a ball of 0.75 m holds about a hundred points"""
    b0 = synth.make_pair_batch(seed, pairs, n, kp, 4, "slab:3")
    rng = np.random.default_rng(seed)
    return dict(anc_pc=b0["src_pc"], pos_pc=b0["dst_pc"], anc_sn=b0["src_sn"], pos_sn=b0["dst_sn"], anc_kp=b0["src_node"],
                pos_kp=b0["dst_node"], anc_sigmas=rng.uniform(0.1, 3.0, (pairs, kp)).astype(np.float32),
                neg_idx=np.roll(np.arange(pairs), 1).astype(np.int64), perm=rng.permutation(n).astype(np.int64))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--samples", type=int, default=448)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--precision", default="f32x2", choices=["f32", "f32x3", "f32x2"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f23_wide_group_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "wide_group_bench needs a GPU"
    ops.set_matmul_mode(args.precision)
    K, C, M, B = args.samples, args.channels, args.keypoints, 2 * args.pairs
    opt = DetectorOptions(surface_normal_len=4, descriptor_len=C, ball_radius=0.75, ball_nsamples=K)
    torch.manual_seed(0)
    st = DescriptorStep(opt, "cuda:0", with_optimizer=True)
    batch = batch_to_device(make_batch(args.pairs, args.points, M), "cuda:0")
    res = {"metric": "f23_wide_group", "device": torch.cuda.get_device_name(0), "host": platform.node(),
           "precision": args.precision, "pairs": args.pairs, "points": args.points, "keypoints": M, "samples": K,
           "channels": C, "radius": 0.75, "positions": B * M * K, "reps": args.reps, "rounds": args.rounds}

    def step(wide):
        ops.WIDE_GROUPS = bool(wide)
        st.step(batch, eager=True)

    meds = {"fused": [], "fallback": []}
    wins = {"fused": [], "fallback": []}
    for _ in range(args.rounds):
        for name, wide in (("fused", True), ("fallback", False)):
            m, w = device_us(lambda: step(wide), args.reps, windows=3, warmup=1)
            meds[name].append(round(m, 1))
            wins[name].append(w)
    res["fused_step_us"], res["fallback_step_us"] = meds["fused"], meds["fallback"]
    res["fused_step_us_windows"], res["fallback_step_us_windows"] = wins["fused"], wins["fallback"]
    res["fused_below_fallback"] = bool(max(meds["fused"]) < min(meds["fallback"]))
    res["fused_peak_bytes"] = peak_bytes(lambda: step(True))
    res["fallback_peak_bytes"] = peak_bytes(lambda: step(False))
    ops.WIDE_GROUPS = True

    # the two kernels alone, on tensors of the step's size: y, dz [B, C, M*K]
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randn((B, C, M, K), device="cuda", generator=g)
    dz = torch.randn((B, C, M * K), device="cuda", generator=g)
    coef = torch.stack([torch.rand(C, device="cuda", generator=g) + 0.5, torch.randn(C, device="cuda", generator=g) * 0.1,
                        torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")]).contiguous()
    rows = B * C * M
    pool_bytes = 4.0 * rows * (K + 3)                                     # y in; pooled, arg, yarg out
    us = device_us(lambda: ops.group_max_wide(y, coef, True, want_yarg=True), 20)
    res["group_max_wide"] = dict(us=round(us[0], 1), us_windows=us[1], bytes=pool_bytes, gb_per_s=round(pool_bytes / us[0] / 1e3, 1))
    y3 = y.view(B, C, M * K)
    red_bytes = 4.0 * (2 * B * C * M * K + 2 * rows)                      # dZ, Y in; the per-neighbourhood sums out
    us = device_us(lambda: ops.bn_backward_reduce_wide(dz, y3, coef, coef[2], coef[3], None, True, K), 20)
    res["bn_backward_reduce_wide"] = dict(us=round(us[0], 1), us_windows=us[1], bytes=red_bytes,
                                          gb_per_s=round(red_bytes / us[0] / 1e3, 1))
    # what the fallback runs in the pooling's place: bn_apply writes the activated tensor, group_max_kernel<64> pools it
    us = device_us(lambda: ops.group_max(ops.bn_apply(y3, coef, True).view(B, C, M, K)), 20)
    res["fallback_apply_then_group_max"] = dict(us=round(us[0], 1), us_windows=us[1])
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
