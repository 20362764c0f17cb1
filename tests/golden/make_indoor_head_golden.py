"""tests/golden/make_indoor_head_golden.py -- regenerates indoor_head.npz: the reference's own DescriptorLiteOldGlobal
(models/networks.py:388-479) + DescCGFLoss (models/losses.py:240-314) and a backward pass, as ModelDescriptorIndoor.optimize
(models/keypoint_descriptor.py:425-467) strings them together, on the CPU over the drop-in modules of make_golden.py.

The reference's class calls operations.ball_query_wrapper, which its models/operations.py holds as a comment only; that
comment states the query DescriptorLiteOld runs in line (networks.py:357-359): the distance matrix, then the first nsamples
indices inside the radius in point order, padded from the first.  This script installs exactly that call on the imported
module, in its own process; nothing of the reference is edited or copied.

Two pairs (four clouds), N = 600 points in a cube of half-extent 0.4, M = 24 keypoints per cloud (fc1 and fc2 take their
BatchNorm statistics over 4 * 24 = 96 positions), K = 448, descriptor_len = 64, radius 0.75, CGF_radius 0.075, gamma 0.3,
sigma_max 0.5.  A positive cloud is its anchor under a known rigid motion with jitter; anchor keypoints are points of the
anchor (the one nearest the centre: a TRUNCATED ball, the one nearest a corner: a PADDED one, 22 others); positive keypoints
are the moved anchors plus noise of at most 0.03 per coordinate, five of them moved by more than 0.2 instead, in a shuffled
order; the sigmas straddle sigma_max.

Recorded while the reference runs: np.random.permutation (replaced by the stored one), the three torch.rand draws of the loss
(proved to be the recorded ones), the three index tensors the loss gathers with, every torch.max route of the forward (both
pools over K and the pool over the keypoints), every ReLU decision within RELU_NEAR of zero, the ball indices.  The script
ASSERTS tests/indoor_oracle.py::fixture_conditions and walks the seeds until they hold.

The same step then runs in float64 at the float32 run's decisions (ball indices, pool routes, ReLU masks and loss indices
replayed): `noise/<parameter>` is the float32 reference's own error against it, max |g32 - g64| / max |g64|, and
`grad64/<parameter>` that run's gradient rounded once to float32.

    python tests/golden/make_indoor_head_golden.py        (needs the reference checkout)
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import indoor_oracle as io_  # noqa: E402

K, N, M, CS, D, RADIUS, PAIRS = 448, 600, 24, 4, 64, 0.75, 2
CGF_RADIUS, GAMMA, SIGMA_MAX = 0.075, 0.3, 0.5


class Recorder:
    """Wraps the entry points the reference's forward calls.  record: keeps the decisions; replay: imposes kept ones."""

    def __init__(self, replay=None):
        self.replay = replay
        self.ball, self.members, self.pools, self.masks, self.near = None, None, [], [], []
        self._at = [0, 0]

    def __enter__(self):
        self.bq = sys.modules["ball_query"]
        self.orig = (self.bq.forward_cuda_shared_mem, torch.max, torch.nn.ReLU.forward)
        orig_bq, orig_max, orig_relu = self.orig
        me = self

        def bq_wrap(d, r_, k):
            if me.replay is not None:
                return torch.from_numpy(me.replay.ball.astype(np.int64))
            r = orig_bq(d, r_, k)
            me.ball = r.numpy().astype(np.int16).copy()
            me.members = (d <= np.float32(r_)).sum(dim=2).numpy().astype(np.int32)     # the query's own comparison
            return r

        def max_wrap(*a, **kw):
            pool = len(a) == 1 and kw.get("dim") == a[0].dim() - 1 and a[0].dim() in (3, 4) and a[0].is_floating_point()
            if not pool:
                return orig_max(*a, **kw)
            dim, keep = kw["dim"], bool(kw.get("keepdim", False))
            if me.replay is not None:
                arg = torch.from_numpy(me.replay.pools[me._at[0]].astype(np.int64))
                me._at[0] += 1
                val = torch.gather(a[0], dim, arg.unsqueeze(dim))
                return (val, arg.unsqueeze(dim)) if keep else (val.squeeze(dim), arg)
            r = orig_max(*a, **kw)
            me.pools.append((r[1].squeeze(dim) if keep else r[1]).numpy().astype(np.int16).copy())
            return r

        def relu_wrap(self_, x):
            if me.replay is not None:
                mask = me.replay.masks[me._at[1]]
                me._at[1] += 1
                return x * mask.to(x.dtype)
            flat = x.detach().reshape(-1)
            idx = torch.nonzero(flat.abs() < mg.RELU_NEAR, as_tuple=False).reshape(-1)
            me.near.append((idx.numpy().astype(np.int32), (flat[idx] > 0).numpy(), int(flat.numel())))
            me.masks.append(x.detach() > 0)
            return orig_relu(self_, x)
        self.bq.forward_cuda_shared_mem, torch.max, torch.nn.ReLU.forward = bq_wrap, max_wrap, relu_wrap
        return self

    def __exit__(self, *exc):
        self.bq.forward_cuda_shared_mem, torch.max, torch.nn.ReLU.forward = self.orig
        return False


def rotation(rng):
    """a rotation by at most ~0.3 rad about a random axis"""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.1, 0.3)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def inputs(rng):
    f = np.float32
    out = {k: [] for k in ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "anc_kp", "pos_kp", "anc_R_pos", "anc_scale_pos",
                           "anc_shift_pos")}
    for _ in range(PAIRS):
        pc = (mg.synth.make_cloud(rng, N, "cube") / f(125.0)).astype(f)                   # half-extent 0.4
        R, t = rotation(rng), rng.uniform(-0.05, 0.05, (3, 1))
        order = rng.permutation(N)
        pos = (R @ pc.astype(np.float64) + t + rng.uniform(-0.004, 0.004, (3, N)))[:, order].astype(f)
        centre, corner = int(np.argmin((pc ** 2).sum(0))), int(np.argmax(pc.sum(0)))
        rest = [int(i) for i in rng.permutation(N) if i not in (centre, corner)][:M - 2]
        kp = np.ascontiguousarray(pc[:, [centre, corner] + rest])
        noise = rng.uniform(-0.03, 0.03, (3, M))
        far = rng.choice(M, 5, replace=False)
        away = rng.standard_normal((3, 5))
        noise[:, far] = away / np.linalg.norm(away, axis=0) * rng.uniform(0.2, 0.3, 5)     # moved by more than 0.2
        pos_kp = (R @ kp.astype(np.float64) + t + noise)[:, rng.permutation(M)].astype(f)
        for k, v in (("anc_pc", pc), ("pos_pc", pos), ("anc_sn", mg.synth.make_normals(rng, N, CS)),
                     ("pos_sn", mg.synth.make_normals(rng, N, CS)), ("anc_kp", kp), ("pos_kp", pos_kp),
                     ("anc_R_pos", R.astype(f)), ("anc_scale_pos", np.ones((1,), f)), ("anc_shift_pos", t.astype(f))):
            out[k].append(v)
    out = {k: np.ascontiguousarray(np.stack(v)).astype(f) for k, v in out.items()}
    out["anc_sigmas"] = rng.uniform(0.05, 0.8, (PAIRS, M)).astype(f)
    out["perm"] = rng.permutation(N).astype(np.int64)
    return out


def step(networks, losses, net, x, dtype, seed, replay=None):
    """ModelDescriptorIndoor.optimize's lines on `net` -> (recorder, results); replay: the float32 run's recorder"""
    opt = net.opt
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    cast = (lambda v: v.to(dtype))
    net.train()
    orig_perm = np.random.permutation
    np.random.permutation = lambda n: x["perm"].copy()
    try:
        with Recorder(replay) as rec:
            desc, x_feat = net(cast(torch.cat((t["anc_pc"], t["pos_pc"]))), cast(torch.cat((t["anc_sn"], t["pos_sn"]))),
                               cast(torch.cat((t["anc_kp"], t["pos_kp"]))), True, None)
    finally:
        np.random.permutation = orig_perm
    anc_d, pos_d = desc[:PAIRS], desc[PAIRS:]
    net.zero_grad()
    # keypoint_descriptor.py:448-450, in float32 whatever the run: the decisions of the loss are float32 ones
    moved = torch.matmul(t["anc_R_pos"], t["anc_kp"])
    moved = moved * t["anc_scale_pos"].unsqueeze(1).unsqueeze(2).reshape(PAIRS, 1, 1)
    moved = moved + t["anc_shift_pos"]
    torch.manual_seed(seed)
    u = (torch.rand((PAIRS, M, M)), torch.rand((PAIRS, M, M)), torch.rand((PAIRS, M)))
    drawn, gathered = [], []
    rand, gather = torch.rand, torch.gather

    def rec_rand(*a, **k):
        drawn.append(rand(*a, **k))
        return drawn[-1]

    def rec_gather(inp, dim, index, **k):
        gathered.append(index.clone())
        return gather(inp, dim, index, **k)
    torch.manual_seed(seed)
    torch.rand, torch.gather = rec_rand, rec_gather
    try:
        trip, active = losses.DescCGFLoss(opt)(moved, anc_d, t["pos_kp"], pos_d, cast(t["anc_sigmas"]))
    finally:
        torch.rand, torch.gather = rand, gather
    assert len(drawn) == 3 and all(torch.equal(a, b) for a, b in zip(drawn, u)), "the class drew other uniforms"
    assert len(gathered) == 3
    loss = torch.mean(trip)
    loss.backward()
    return rec, dict(desc=desc, x_feat=x_feat, trip=trip, active=active, loss=loss, moved=moved, u=u,
                     sel=torch.cat(gathered, dim=2).numpy().astype(np.int32))


def attempt(networks, losses, seed):
    rng = np.random.default_rng(seed)
    x = inputs(rng)
    opt = mg.Opt(surface_normal_len=CS, descriptor_len=D, ball_radius=RADIUS, ball_nsamples=K, CGF_radius=CGF_RADIUS,
                 triple_loss_gamma=GAMMA, sigma_max=SIGMA_MAX)
    net = networks.DescriptorLiteOldGlobal(opt)
    mg.load_filled(net)
    net64 = copy.deepcopy(net).double()
    rec, r = step(networks, losses, net, x, torch.float32, seed)
    assert tuple(r["x_feat"].shape) == (2 * PAIRS, 3 + CS, M, K) and len(rec.pools) == 3 and len(rec.near) == 6
    assert len(net.state_dict()) == 46
    _, has, take_far = io_.co.select(r["moved"].numpy(), x["pos_kp"], CGF_RADIUS, *(v.numpy() for v in r["u"]))
    out = dict(x, anc_kp_moved=r["moved"].numpy(), u1=r["u"][0].numpy(), u2=r["u"][1].numpy(), u3=r["u"][2].numpy(),
               descriptors=r["desc"].detach().numpy(), triplet=r["trip"].detach().numpy(), active=r["active"].numpy(),
               loss=r["loss"].detach().numpy(), ball_members=rec.members, seed=np.int64(seed),
               cfg_ball_nsamples=np.int32(K), cfg_ball_radius=np.float32(RADIUS), cfg_descriptor_len=np.int32(D),
               cfg_CGF_radius=np.float64(CGF_RADIUS), cfg_triple_loss_gamma=np.float64(GAMMA),
               cfg_sigma_max=np.float64(SIGMA_MAX))
    out.update({"idx/sel": r["sel"], "idx/has": has, "idx/take_far": take_far, "idx/ball_idx": rec.ball})
    for i, p in enumerate(rec.pools):
        out["idx/pool_arg_%d" % i] = p
    for i, (idx, on, numel) in enumerate(rec.near):
        out["idx/relu_near_idx_%d" % i], out["idx/relu_near_on_%d" % i], out["idx/relu_numel_%d" % i] = idx, on, np.int64(numel)
    try:
        figures = io_.fixture_conditions(out)
    except AssertionError as e:
        print("seed %d: %s" % (seed, e))
        return None
    assert np.isfinite(out["triplet"]).all()
    out.update(mg.grad_digest(net))
    out.update({"grad/" + k: p.grad.detach().numpy().copy() for k, p in net.named_parameters()})
    for k, v in net.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["buf/" + k] = v.numpy().copy()
    # the same module in evaluation mode, on the buffers the step left
    net.eval()
    orig_perm = np.random.permutation
    np.random.permutation = lambda n: x["perm"].copy()
    try:
        with torch.no_grad():
            out["descriptors_eval"] = net(torch.from_numpy(np.concatenate([x["anc_pc"], x["pos_pc"]])),
                                          torch.from_numpy(np.concatenate([x["anc_sn"], x["pos_sn"]])),
                                          torch.from_numpy(np.concatenate([x["anc_kp"], x["pos_kp"]])), False, None)[0].numpy()
    finally:
        np.random.permutation = orig_perm
    # float64 at the float32 run's decisions: the reference's own float32 noise
    _, r64 = step(networks, losses, net64, x, torch.float64, seed, replay=rec)
    assert np.array_equal(r64["sel"], r["sel"])
    p64 = dict(net64.named_parameters())
    for k, p in net.named_parameters():
        g64 = p64[k].grad.numpy()
        out["noise/" + k] = np.float64(np.abs(p.grad.numpy().astype(np.float64) - g64).max() / max(np.abs(g64).max(), 1e-30))
        out["grad64/" + k] = g64.astype(np.float32)         # the float64 gradient, stored rounded once (6e-8: far below the bars)
    for k, a, b in (("descriptors", r["desc"], r64["desc"]), ("triplet", r["trip"], r64["trip"]), ("loss", r["loss"], r64["loss"])):
        b = b.detach().numpy()
        out["noise/" + k] = np.float64(np.abs(a.detach().numpy().astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
    print("seed %d: %s  loss %.6f  worst gradient noise %.2e" % (
        seed, figures, float(out["loss"]), max(float(v) for k, v in out.items() if k.startswith("noise/") and "." in k)))
    return out


def main():
    _, networks, losses, _, _ = mg.import_reference()
    bq = sys.modules["ball_query"]
    networks.operations.ball_query_wrapper = lambda pc, node, r, k: bq.forward_cuda_shared_mem(
        torch.norm(node.unsqueeze(3) - pc.unsqueeze(2), p=2, dim=1).detach(), r, k).long()
    for seed in range(1, 100):
        out = attempt(networks, losses, seed)
        if out is not None:
            mg.save("indoor_head.npz", **out)
            return
    raise SystemExit("no seed satisfies the fixture's conditions")


if __name__ == "__main__":
    main()
