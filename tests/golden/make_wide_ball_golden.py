"""tests/golden/make_wide_ball_golden.py -- regenerates descriptor_wide_ball.npz: the reference's own DescriptorLiteOld +
DescPairScanLoss at the indoor neighbourhood size, ball_nsamples = 448 (scenenn/options_descriptor.py), on the CPU over the
drop-in modules of make_golden.py (whose gen_descriptor has its shape written in and stores pool routes as int8).

One pair (two clouds), N = 600 points in a cube of half-extent 0.4, M = 3 keypoints per cloud, descriptor_len = 64, radius
0.75.  Keypoint 0 is the point nearest the centre (every point lies within 0.75 of it: its ball is TRUNCATED to the first 448
of the permuted cloud), keypoint 1 the point nearest a corner (fewer than 448 members: its ball is PADDED, its members
repeated from the first on), keypoint 2 any point.  Both conditions are asserted here, on the CPU.

Stored: the inputs, the recorded permutation, the BatchNorm buffers after the step (the parameters are
usip_amd.synth.fill_parameters of the state dict's shapes), descriptors, triplet terms, loss, EVERY parameter gradient in full
and its digests, the ball indices, both pool routes (int16) and the near-zero ReLU decisions of conv1..conv4.  Data only.

    python tests/golden/make_wide_ball_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

K, N, M, CS, D, RADIUS = 448, 600, 3, 4, 64, 0.75


def capture():
    """mg.capture_indices for neighbourhoods wider than an int8: ball indices, the max-pool routes and the near-zero ReLU
    decisions, recorded by wrapping the entry points the reference's forward calls"""
    rec = {}
    bq = sys.modules["ball_query"]
    orig_bq, orig_max, orig_relu = bq.forward_cuda_shared_mem, torch.max, torch.nn.ReLU.forward

    def bq_wrap(d, r_, k):
        r = orig_bq(d, r_, k)
        rec["ball_idx"] = r.numpy().astype(np.int16).copy()
        rec["ball_members"] = (d <= np.float32(r_)).sum(dim=2).numpy().astype(np.int32)       # the query's own comparison
        return r

    def max_wrap(*a, **kw):
        r = orig_max(*a, **kw)
        if kw.get("dim") == 3 and len(a) == 1 and a[0].dim() == 4:
            arg = r[1].reshape(a[0].shape[0], a[0].shape[1], a[0].shape[2])
            rec["pool_arg_%d" % sum(k.startswith("pool_arg_") for k in rec)] = arg.numpy().astype(np.int16).copy()
        return r

    def relu_wrap(self, x):
        i = sum(k.startswith("relu_near_idx_") for k in rec)
        flat = x.detach().reshape(-1)
        idx = torch.nonzero(flat.abs() < mg.RELU_NEAR, as_tuple=False).reshape(-1)
        rec["relu_near_idx_%d" % i] = idx.numpy().astype(np.int32)
        rec["relu_near_on_%d" % i] = (flat[idx] > 0).numpy()
        rec["relu_numel_%d" % i] = np.int64(flat.numel())
        return orig_relu(self, x)
    bq.forward_cuda_shared_mem, torch.max, torch.nn.ReLU.forward = bq_wrap, max_wrap, relu_wrap

    def restore():
        bq.forward_cuda_shared_mem, torch.max, torch.nn.ReLU.forward = orig_bq, orig_max, orig_relu
    return rec, restore


def cloud(rng):
    pc = (mg.synth.make_cloud(rng, N, "cube") / np.float32(125.0)).astype(np.float32)         # half-extent 0.4
    centre = int(np.argmin((pc ** 2).sum(0)))
    corner = int(np.argmax(pc.sum(0)))
    other = int(rng.integers(0, N))
    return pc, np.ascontiguousarray(pc[:, [centre, corner, other]])


def main():
    _, networks, losses, _, _ = mg.import_reference()
    rng = np.random.default_rng(448)
    opt = mg.Opt(surface_normal_len=CS, descriptor_len=D, ball_radius=RADIUS, ball_nsamples=K, triple_loss_gamma=0.5,
                 sigma_max=3.0)
    (anc, anc_kp), (pos, pos_kp) = cloud(rng), cloud(rng)
    anc, pos, anc_kp, pos_kp = anc[None], pos[None], anc_kp[None], pos_kp[None]
    anc_sn, pos_sn = mg.synth.make_normals(rng, N, CS)[None], mg.synth.make_normals(rng, N, CS)[None]
    anc_sigmas = rng.uniform(0.1, 3.5, (1, M)).astype(np.float32)
    neg_idx = np.array([0], dtype=np.int64)                  # one pair: the negative scan is the anchor's own
    perm = rng.permutation(N).astype(np.int64)
    net = networks.DescriptorLiteOld(opt)
    mg.load_filled(net)
    net.train()
    orig = np.random.permutation
    np.random.permutation = lambda n: perm.copy()
    rec, restore = capture()
    try:
        desc, x_feat = net(torch.from_numpy(np.concatenate([anc, pos])), torch.from_numpy(np.concatenate([anc_sn, pos_sn])),
                           torch.from_numpy(np.concatenate([anc_kp, pos_kp])), True, None)
    finally:
        np.random.permutation = orig
        restore()
    members = rec.pop("ball_members")
    assert tuple(x_feat.shape) == (2, 3 + CS, M, K) and tuple(members.shape) == (2, M)
    assert (members >= K).any(), "no truncated ball: %s" % members.tolist()
    assert ((members > 0) & (members < K)).any(), "no padded ball: %s" % members.tolist()
    anc_d, pos_d = desc[:1], desc[1:]
    net.zero_grad()
    trip, active = losses.DescPairScanLoss(opt)(anc_d, pos_d, anc_d[torch.from_numpy(neg_idx), :, :],
                                                torch.from_numpy(anc_sigmas))
    loss = torch.mean(trip)
    loss.backward()
    out = dict(anc_pc=anc, pos_pc=pos, anc_sn=anc_sn, pos_sn=pos_sn, anc_kp=anc_kp, pos_kp=pos_kp, anc_sigmas=anc_sigmas,
               neg_idx=neg_idx, perm=perm, descriptors=desc.detach().numpy(), triplet=trip.detach().numpy(),
               active=active.numpy(), loss=loss.detach().numpy(), ball_members=members,
               cfg_ball_nsamples=np.int32(K), cfg_ball_radius=np.float32(RADIUS), cfg_descriptor_len=np.int32(D))
    out.update(mg.grad_digest(net))
    out.update({"grad/" + k: p.grad.detach().numpy().copy() for k, p in net.named_parameters()})
    out.update({"idx/" + k: v for k, v in rec.items()})
    for k, v in net.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["buf/" + k] = v.numpy().copy()
    mg.save("descriptor_wide_ball.npz", **out)
    print("members per ball:", members.tolist(), " loss", float(loss.detach()))


if __name__ == "__main__":
    main()
