#!/usr/bin/env python
"""Times of the indoor descriptor's training step at its own shape (scenenn/options_descriptor.py: 2 pairs, 5000 points, 512
keypoints, balls of 448 samples, descriptor_len 128): forward + backward + Adam of usip_amd.step.IndoorDescriptorStep (the head
with the global context + the CGF triplet loss) and, beside it in the same process, of usip_amd.step.DescriptorStep
(DescriptorLiteOld + the pair-scan loss) at the same shape -- the difference is what the tail costs.  Then the two launches of
csrc/unit_columns.hip stand-alone against the torch expression they replace, the per-kernel rows of the tail from usip_amd.prof
over one instrumented step, and the peak device memory of a step.  ONE JSON line, also written to --out.  No ratio is asserted.

    python tools/indoor_step_bench.py [--rounds 4] [--reps 5] [--precision f32x2] [--out profiles/f25_indoor_step_bench.json]

Step times: events on the launch stream around `reps` back-to-back eager steps after a warm-up, the median of three windows;
`rounds` alternating rounds (indoor, outdoor, indoor, ...), every round's median and windows listed."""
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
from usip_amd import functional as Fh                        # noqa: E402
from usip_amd import ops, prof, synth                        # noqa: E402
from usip_amd.networks import IndoorOptions                  # noqa: E402
from usip_amd.step import DescriptorStep, IndoorDescriptorStep, batch_to_device   # noqa: E402
from iss_bench import device_us                              # noqa: E402
from wide_group_bench import peak_bytes                      # noqa: E402

TAIL = ("group_max", "group_max_wide", "shared_mlp_gemm_fwd_pooled", "shared_mlp_gemm_dgrad_pooled", "unit_columns",
        "unit_columns_backward", "cgf_select", "cgf_loss", "cgf_loss_backward", "rigid_transform")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f25_indoor_step_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "indoor_step_bench needs a GPU"
    ops.set_matmul_mode(args.precision)
    K, C, M, B = args.samples, args.channels, args.keypoints, 2 * args.pairs
    opt = IndoorOptions(descriptor_len=C, ball_nsamples=K, input_pc_num=args.points, node_num=M, batch_size=args.pairs)
    torch.manual_seed(0)
    indoor = IndoorDescriptorStep(opt, "cuda:0", with_optimizer=True)
    outdoor = DescriptorStep(opt, "cuda:0", with_optimizer=True)
    rng = np.random.default_rng(25)
    batch_np = synth.make_indoor_pair_batch(25, args.pairs, args.points, M, 4)
    batch_np["perm"] = rng.permutation(args.points).astype(np.int64)
    batch = batch_to_device(batch_np, "cuda:0")
    batch_out = dict({k: batch[k] for k in ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "anc_kp", "pos_kp", "anc_sigmas", "perm")},
                     neg_idx=torch.from_numpy(np.roll(np.arange(args.pairs), 1).astype(np.int64)).to("cuda:0"))
    res = {"metric": "f25_indoor_step", "device": torch.cuda.get_device_name(0), "host": platform.node(),
           "precision": args.precision, "pairs": args.pairs, "points": args.points, "keypoints": M, "samples": K,
           "channels": C, "radius": opt.ball_radius, "keypoint_pool_path": Fh._group_path(M), "reps": args.reps,
           "rounds": args.rounds}
    forms = (("indoor", lambda: indoor.step(batch, eager=True)), ("outdoor", lambda: outdoor.step(batch_out, eager=True)))
    meds, wins = {n: [] for n, _ in forms}, {n: [] for n, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            m, w = device_us(fn, args.reps, windows=3, warmup=1)
            meds[name].append(round(m, 1))
            wins[name].append(w)
    for name, _ in forms:
        res[name + "_step_us"], res[name + "_step_us_windows"] = meds[name], wins[name]
    res["indoor_peak_bytes"] = peak_bytes(forms[0][1])
    res["outdoor_peak_bytes"] = peak_bytes(forms[1][1])
    res["indoor_loss"], res["indoor_active"] = float(indoor.last["loss"].detach()), float(indoor.last["active_percentage"])

    # the normalisation alone, on a tensor of the step's size, against the expression DescriptorLiteOld keeps
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((B, C, M), device="cuda", generator=g)
    cot = torch.randn((B, C, M), device="cuda", generator=g)
    _, norm = ops.unit_columns(x)
    us = device_us(lambda: ops.unit_columns(x), 50)
    res["unit_columns"] = dict(us=round(us[0], 1), us_windows=us[1], bytes=8.0 * B * C * M)
    us = device_us(lambda: ops.unit_columns_backward(cot, x, norm), 50)
    res["unit_columns_backward"] = dict(us=round(us[0], 1), us_windows=us[1], bytes=12.0 * B * C * M)
    us = device_us(lambda: x / (torch.norm(x, dim=1, keepdim=True) + 1e-5), 50)
    res["torch_forward"] = dict(us=round(us[0], 1), us_windows=us[1])
    xr = x.clone().requires_grad_(True)

    def torch_both():
        xr.grad = None
        (xr / (torch.norm(xr, dim=1, keepdim=True) + 1e-5)).backward(cot)
    us = device_us(torch_both, 50)
    res["torch_forward_backward"] = dict(us=round(us[0], 1), us_windows=us[1])
    us = device_us(lambda: ops.unit_columns_backward(cot, x, ops.unit_columns(x)[1]), 50)
    res["unit_columns_forward_backward"] = dict(us=round(us[0], 1), us_windows=us[1])

    # the tail's kernels inside one instrumented step (events around every launch: the sum is not the step's time)
    prof.reset()
    prof.enable(True)
    try:
        indoor.step(batch, eager=True)
        rows = prof.summary()
    finally:
        prof.enable(False)
        prof.reset()
    res["tail_kernels"] = {k: dict(calls=v["calls"], avg_us=round(v["avg_us"], 1), key=v["rocprof_key"])
                           for k, v in sorted(rows.items()) if k.startswith(TAIL) or "pooled" in k}
    res["instrumented_step_kernel_us"] = round(sum(v["total_ms"] for v in rows.values()) * 1e3, 1)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
