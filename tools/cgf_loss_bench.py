#!/usr/bin/env python
"""Times of the f-22 CGF triplet loss (usip_amd.losses.DescCGFLoss) at the indoor model's own shape (scenenn/
options_descriptor.py: node_num 512, descriptor_len 128): forward + backward of loss.mean() at B = 2 and B = 8, M = 512, C = 128,
on the Philox path.  Beside it, in the same process: this tool's own dense torch restatement of the reference's formulation
(models/losses.py:240-314: the B x C x M x M difference tensor, the B x M x M norm, three torch.rand matrices) in float32 on
the device, and the library's host twin on `--threads` threads; and the peak device memory of both device forms.  ONE JSON line,
also written to --out.  No ratio is asserted anywhere.

    python tools/cgf_loss_bench.py [--reps 20] [--threads 16] [--skip-host] [--out profiles/f22_cgf_loss_bench.json]

Device times: events on the launch stream around `reps` back-to-back forward + backward calls after a warm-up, median of 5
windows, all five listed.  The fused form is also timed per stage (selection, loss, backward) through the tensor-level wrappers.
The host twin is timed on the wall clock, median of 5.  Peak memory: torch.cuda.max_memory_allocated over one call, above what
the inputs hold."""
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
from usip_amd import ops                        # noqa: E402
from usip_amd.losses import DescCGFLoss        # noqa: E402
from iss_bench import device_us, wall_ms        # noqa: E402

RADIUS, GAMMA, SIGMA_MAX = 0.075, 0.3, 0.5      # scenenn/options_descriptor.py


class Opt:
    CGF_radius, triple_loss_gamma, sigma_max = RADIUS, GAMMA, SIGMA_MAX


def dense_reference(anc_kp, anc_desc, pos_kp, pos_desc, anc_sigma):
    """the reference's formulation, densely, with its own torch.rand draws"""
    B, M = anc_kp.shape[0], anc_kp.shape[2]
    ddiff = torch.norm(anc_desc.unsqueeze(3) - pos_desc.unsqueeze(2), dim=1)
    kdiff = torch.norm(anc_kp.unsqueeze(3) - pos_kp.unsqueeze(2), dim=1)
    pos_mask = kdiff <= RADIUS
    has = pos_mask.any(dim=2).float()
    nearby = torch.max(pos_mask.float() * torch.rand((B, M, M), device=anc_kp.device), dim=2, keepdim=True)[1]
    d_pos = torch.gather(ddiff, 2, nearby).squeeze(2)
    far = torch.min(kdiff + pos_mask.float() * 1000, dim=2, keepdim=True)[1]
    d_far = torch.gather(ddiff, 2, far).squeeze(2)
    outside = torch.max(torch.rand((B, M, M), device=anc_kp.device) * (kdiff > RADIUS).float(), dim=2, keepdim=True)[1]
    d_out = torch.gather(ddiff, 2, outside).squeeze(2)
    pick = (torch.rand((B, M), device=anc_kp.device) < 0.5).float()
    d_neg = pick * d_far + (1 - pick) * d_out
    n1 = has.sum(dim=1) + 1
    before = (d_pos - d_neg + GAMMA) * has
    active = (before > 1e-5).float().sum(dim=1) / n1
    w = torch.clamp(SIGMA_MAX - anc_sigma, min=0)
    w = (w / w.mean(dim=1, keepdim=True)).detach()
    return w * torch.clamp(before, min=0) * (M / n1).detach().unsqueeze(1), active


def batch(B, M, C, seed):
    """keypoints on a 3 m x 3 m x 0.3 m slab, the positives a shuffled copy moved by up to 0.04 m: most anchors have a match"""
    g = np.random.default_rng(seed)
    anc = g.uniform(-1.5, 1.5, (B, 3, M))
    anc[:, 2] *= 0.1
    pos = np.stack([(anc[b] + g.uniform(-0.04, 0.04, (3, M)))[:, g.permutation(M)] for b in range(B)])
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)      # noqa: E731   descriptors are unit vectors
    f = np.float32
    return [torch.from_numpy(np.ascontiguousarray(a.astype(f))) for a in
            (anc, unit(g.standard_normal((B, C, M))), pos, unit(g.standard_normal((B, C, M))), g.uniform(0.0, 0.6, (B, M)))]


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f22_cgf_loss_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cgf_loss_bench needs a GPU"
    M, C = args.nodes, args.channels
    res = {"metric": "f22_cgf_loss", "device": torch.cuda.get_device_name(0), "host": platform.node(), "nodes": M, "channels": C,
           "radius": RADIUS, "gamma": GAMMA, "sigma_max": SIGMA_MAX, "reps": args.reps, "shapes": {}}
    for B in (2, 8):
        host = batch(B, M, C, 22 + B)
        t = [x.cuda() for x in host]
        t[1].requires_grad_(True)
        t[3].requires_grad_(True)
        mod = DescCGFLoss(Opt, seed=1)

        def fused():
            t[1].grad = t[3].grad = None
            loss, _ = mod(*t)
            loss.mean().backward()

        def dense():
            t[1].grad = t[3].grad = None
            loss, _ = dense_reference(*t)
            loss.mean().backward()

        r = {}
        r["fused_fwd_bwd_us"], r["fused_fwd_bwd_us_all"] = device_us(fused, args.reps)
        r["dense_fwd_bwd_us"], r["dense_fwd_bwd_us_all"] = device_us(dense, args.reps)
        r["fused_fwd_bwd_us_again"] = device_us(fused, args.reps)[0]     # alternated: the spread between two windows of one form
        r["dense_fwd_bwd_us_again"] = device_us(dense, args.reps)[0]
        r["fused_peak_bytes"], r["dense_peak_bytes"] = peak_bytes(fused), peak_bytes(dense)
        # the stages of the fused form through the tensor-level wrappers
        kp_a, d_a, kp_p, d_p, sg = [x.detach() for x in t]
        sel, has, tf = ops.cgf_select(kp_a, kp_p, RADIUS, None, 1, 0)
        loss, active, dist, coef = ops.cgf_loss(d_a, d_p, sg, sel, has, tf, GAMMA, SIGMA_MAX)
        g = torch.full_like(loss, 1.0 / loss.numel())
        r["select_us"] = device_us(lambda: ops.cgf_select(kp_a, kp_p, RADIUS, None, 1, 0), args.reps)[0]
        r["loss_us"] = device_us(lambda: ops.cgf_loss(d_a, d_p, sg, sel, has, tf, GAMMA, SIGMA_MAX), args.reps)[0]
        r["backward_us"] = device_us(lambda: ops.cgf_loss_backward(d_a, d_p, sel, tf, dist, coef, g), args.reps)[0]
        r["matched_share"] = float(has.float().mean())
        r["active_mean"] = float(active.mean())
        if not args.skip_host:
            def twin():
                s = ops.cgf_select_cpu(host[0], host[2], RADIUS, None, 1, 0, 0, args.threads)
                out = ops.cgf_loss_cpu(host[1], host[3], host[4], *s, GAMMA, SIGMA_MAX, args.threads)
                ops.cgf_loss_backward_cpu(host[1], host[3], s[0], s[2], out[2], out[3], g.cpu(), args.threads)
                return s, out
            r["host_threads"] = args.threads
            r["host_twin_fwd_bwd_ms"] = wall_ms(twin)
            s, out = twin()
            r["sel_equals_host"] = bool(torch.equal(sel.cpu(), s[0]) and torch.equal(tf.cpu(), s[2]))
            r["loss_equals_host_bits"] = bool(torch.equal(loss.cpu().view(torch.int32), out[0].view(torch.int32)))
        res["shapes"]["B%d" % B] = r
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
