"""Fixtures of the indoor descriptor's CGF triplet loss: tests/golden/cgf_loss_cases.npz.

Runs the reference's OWN losses.DescCGFLoss (models/losses.py:240-314) on the CPU.  torch is seeded and the three torch.rand
calls the class will make are recorded first, in its order and shapes (B x M x M, B x M x M, B x M); torch is reseeded and the
class runs.  While it runs, torch.rand and torch.gather are wrapped by recorders: the first proves that the class drew
exactly the recorded uniforms, the second hands over the three index tensors the class gathered with -- the reference's own
(j_pos, j_far, j_out).  Stored per case: inputs, draws, loss, active, the descriptor gradients of loss.mean(), the indices.

The script ASSERTS what the fixture needs, so that the reference alone satisfies it, and walks the seeds until all hold:
  * no |d_ij - radius| / radius below 1e-3 (d in float64): rounding can never flip a radius decision;
  * the float32 restatement of the contract (tests/cgf_oracle.py, sqrt((dx dx + dy dy) + dz dz), first arg-max / arg-min)
    selects the reference's three indices for every anchor -- the all-inside element included, whose j_far is decided by the
    float32 quantisation of d + 1000;
  * no recorded uniform is exactly 0.
The seed each case settled on is stored with it.

    python tests/golden/make_cgf_golden.py        (needs the reference checkout)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cgf_oracle as co  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "cgf_loss_cases.npz")
MARGIN = 1e-3
# name: (B, M, C, radius, gamma, sigma_max, the extent of the keypoints, what each batch element is)
CASES = {
    "batch3": (3, 48, 16, 1.0, 0.5, 1.0, 4.0, ("mixed", "none", "inside")),
    "single": (2, 1, 16, 1.0, 0.5, 1.0, 4.0, ("paired", "none")),
    "surface": (2, 48, 16, 0.075, 0.3, 0.5, 0.3, ("mixed", "mixed")),      # scenenn/options_descriptor.py's radius, gamma, sigma_max
    "wide": (2, 40, 24, 5.0, 0.3, 0.5, 20.0, ("mixed", "paired")),
}


class Opt:
    def __init__(self, radius, gamma, sigma_max):
        self.CGF_radius, self.triple_loss_gamma, self.sigma_max = radius, gamma, sigma_max


def reference_losses():
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(REF, "models", "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(g, B, M, C, radius, extent, kinds):
    anc = g.uniform(-extent / 2, extent / 2, (B, 3, M))
    pos = np.zeros_like(anc)
    for b, kind in enumerate(kinds):
        if kind == "mixed":                  # a shuffled copy, half of it near its anchor and half of it a radius or more away
            near = g.uniform(-1, 1, (3, M)) * radius * 0.4
            far = g.uniform(-1, 1, (3, M)) * radius * 3
            pos[b] = (anc[b] + np.where(np.arange(M) % 2 == 0, near, far))[:, g.permutation(M)]
        elif kind == "paired":
            pos[b] = anc[b] + g.uniform(-1, 1, (3, M)) * radius * 0.4
        elif kind == "none":                 # nothing within the radius
            pos[b] = anc[b] + 100.0 * radius
        elif kind == "inside":               # both clouds inside a ball of diameter 0.9 radius: every pair is a positive
            anc[b] = g.uniform(-1, 1, (3, M)) * radius * 0.25
            pos[b] = g.uniform(-1, 1, (3, M)) * radius * 0.25
    f = np.float32
    return dict(anc_kp=anc.astype(f), pos_kp=pos.astype(f), anc_desc=g.standard_normal((B, C, M)).astype(f),
                pos_desc=g.standard_normal((B, C, M)).astype(f),
                anc_sigma=g.uniform(0.0, 1.3, (B, M)).astype(f))    # times sigma_max below: some weights clamp to 0


def run_case(losses, name, seed):
    B, M, C, radius, gamma, sigma_max, extent, kinds = CASES[name]
    x = inputs(np.random.default_rng(seed), B, M, C, radius, extent, kinds)
    x["anc_sigma"] = (x["anc_sigma"] * np.float32(sigma_max)).astype(np.float32)
    torch.manual_seed(seed)
    u1, u2, u3 = torch.rand((B, M, M)), torch.rand((B, M, M)), torch.rand((B, M))
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    t["anc_desc"].requires_grad_(True)
    t["pos_desc"].requires_grad_(True)
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
        loss, active = losses.DescCGFLoss(Opt(radius, gamma, sigma_max))(t["anc_kp"], t["anc_desc"], t["pos_kp"], t["pos_desc"],
                                                                          t["anc_sigma"])
    finally:
        torch.rand, torch.gather = rand, gather
    loss.mean().backward()
    assert len(drawn) == 3 and all(torch.equal(a, b) for a, b in zip(drawn, (u1, u2, u3))), "the class drew other uniforms"
    assert len(gathered) == 3
    ref_sel = torch.cat(gathered, dim=2).numpy().astype(np.int32)                   # (j_pos, j_far, j_out)
    # the three conditions
    d64 = np.sqrt(((x["anc_kp"].astype(np.float64)[:, :, :, None] - x["pos_kp"].astype(np.float64)[:, :, None, :]) ** 2).sum(1))
    margin = float(np.abs(d64 - radius).min() / radius)
    sel, has, take_far = co.select(x["anc_kp"], x["pos_kp"], radius, u1.numpy(), u2.numpy(), u3.numpy())
    ok = margin >= MARGIN and np.array_equal(sel, ref_sel) and all(float(u.min()) > 0.0 for u in (u1, u2, u3))
    if not ok:
        return None
    for b, kind in enumerate(kinds):                                                # the elements are what their names say
        n = int(has[b].sum())
        assert {"none": n == 0, "inside": bool((d64[b] <= radius).all()), "paired": n == M,
                "mixed": 0 < n and not (d64[b] <= radius).all()}[kind], (name, b, kind, n)
    assert np.isfinite(loss.detach().numpy()).all()
    out = dict(x, u1=u1.numpy(), u2=u2.numpy(), u3=u3.numpy(), loss=loss.detach().numpy(), active=active.detach().numpy(),
               d_anc=t["anc_desc"].grad.numpy(), d_pos=t["pos_desc"].grad.numpy(), sel=ref_sel, has=has, take_far=take_far,
               radius=np.float64(radius), gamma=np.float64(gamma), sigma_max=np.float64(sigma_max), seed=np.int64(seed),
               margin=np.float64(margin))
    return {"%s_%s" % (name, k): v for k, v in out.items()}


def main():
    torch.set_num_threads(1)
    losses = reference_losses()
    store = {}
    for name in CASES:
        for seed in range(1, 200):
            got = run_case(losses, name, seed)
            if got is not None:
                print("%s: seed %d, margin %.3e" % (name, seed, float(got[name + "_margin"])))
                store.update(got)
                break
        else:
            raise SystemExit("%s: no seed satisfies the fixture's conditions" % name)
    np.savez(OUT, **store)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
