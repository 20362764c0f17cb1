"""What the tests of the indoor descriptor head (usip_amd.networks.DescriptorLiteOldGlobal, usip_amd.step.IndoorDescriptorStep)
share, and what tests/golden/make_indoor_head_golden.py asserts before it writes tests/golden/indoor_head.npz.  numpy and
torch only; no code shared with the library.

  unit_forward / unit_backward   the unit normalisation of include/usip_hip.h f-25, restated on numpy scalars in the
                                 contract's order (one IEEE operation at a time: held to EQUALITY)
  fixture_conditions             the conditions the fixture must satisfy, from the stored arrays alone
  head_tail                      the head behind conv5's pool (max over the keypoints, concat, fc1..fc3, unit columns) in torch,
                                 any dtype, for autograd
"""
import numpy as np

import cgf_oracle as co

F = np.float32
MARGIN = 1e-3                      # no keypoint distance closer to the CGF radius than this, relative (make_cgf_golden.py)


# ---------------------------------------------------------------------------------------------------- f-25 restated
def unit_forward(x, eps):
    """x f32 [B,C,M] -> (out f32 [B,C,M], norm f32 [B,M]): float64 sum of squares in ascending c, one float32 sqrt result, a
    float32 add, float32 divisions"""
    x = np.asarray(x, F)
    B, C, M = x.shape
    s = np.zeros((B, M), np.float64)
    with np.errstate(all="ignore"):
        for c in range(C):
            v = x[:, c, :].astype(np.float64)
            s = s + v * v
        n = np.sqrt(s).astype(F)
        t = (n + F(eps)).astype(F)
        out = (x / t[:, None, :]).astype(F)
    return out, n


def unit_backward(g, x, n, eps):
    """-> dx f32 [B,C,M]: dot in ascending c; dx = (float)(g / t - (x * dot) / ((n * t) * t)), (float)(g / t) where n == 0"""
    g, x, n = np.asarray(g, F), np.asarray(x, F), np.asarray(n, F)
    B, C, M = x.shape
    dot = np.zeros((B, M), np.float64)
    with np.errstate(all="ignore"):
        for c in range(C):
            dot = dot + g[:, c, :].astype(np.float64) * x[:, c, :].astype(np.float64)
        t = (n + F(eps)).astype(F)
        T, N = t.astype(np.float64)[:, None, :], n.astype(np.float64)[:, None, :]
        direct = g.astype(np.float64) / T
        full = direct - (x.astype(np.float64) * dot[:, None, :]) / ((N * T) * T)
        return np.where((n == 0)[:, None, :], direct, full).astype(F)


# ---------------------------------------------------------------------------------------------------- the fixture's conditions
def fixture_conditions(g):
    """g: the arrays of indoor_head.npz (or the generator's dict before it is written) -> a dict of figures; raises
    AssertionError when a condition does not hold."""
    K, radius = int(g["cfg_ball_nsamples"]), float(g["cfg_CGF_radius"])
    members = np.asarray(g["ball_members"])
    assert (members >= K).any(), "no truncated ball"
    assert ((members > 0) & (members < K)).any(), "no padded ball"
    sel, has, take_far = co.select(g["anc_kp_moved"], g["pos_kp"], radius, g["u1"], g["u2"], g["u3"])
    assert np.array_equal(sel, g["idx/sel"]), "the float32 restatement selects other indices than the reference"
    assert np.array_equal(has, g["idx/has"]) and np.array_equal(take_far, g["idx/take_far"])
    for b in range(has.shape[0]):
        assert has[b].any() and not has[b].all(), "batch element %d has no matched or no unmatched anchor" % b
        assert float(g["active"][b]) > 0.0, "batch element %d has no active triplet" % b
    a, p = np.asarray(g["anc_kp_moved"], np.float64), np.asarray(g["pos_kp"], np.float64)
    d64 = np.sqrt(((a[:, :, :, None] - p[:, :, None, :]) ** 2).sum(1))
    margin = float(np.abs(d64 - radius).min() / radius)
    assert margin >= MARGIN, "a keypoint distance within %.1e of the radius" % margin
    assert all(float(np.asarray(g[k]).min()) > 0.0 for k in ("u1", "u2", "u3")), "a recorded uniform is exactly 0"
    sig = np.asarray(g["anc_sigmas"])
    assert (sig < float(g["cfg_sigma_max"])).any() and (sig > float(g["cfg_sigma_max"])).any(), "the sigmas do not straddle sigma_max"
    return dict(margin=margin, matched=has.sum(axis=1).tolist(), members=members.tolist())


# ---------------------------------------------------------------------------------------------------- the head's tail in torch
def head_tail(d, P, training=True, eps=1e-5, spread=None):
    """d [B,C,M]: the max over K of conv5's output; P: {state_dict key: tensor} of fc1..fc3 in d's dtype -> descriptor [B,C,M]
    as models/networks.py:471-477 writes it (batch statistics when training, the running ones otherwise; buffers untouched).
    spread: a list that receives, per BatchNorm layer, the worst channel's mean^2 / variance over the batch -- how many times
    its statistics amplify a rounding of the layer's output"""
    import torch
    import torch.nn.functional as Fn
    B, C, M = d.shape
    glob = torch.max(d, dim=2, keepdim=True)[0]
    h = torch.cat((d, glob.expand(B, C, M)), dim=1)
    for name in ("fc1", "fc2"):
        h = Fn.conv1d(h, P[name + ".conv.weight"], P[name + ".conv.bias"])
        if spread is not None:
            flat = h.detach().transpose(0, 1).reshape(h.shape[1], -1).double()
            spread.append(float((flat.mean(1) ** 2 / flat.var(1, unbiased=False)).max()))
        h = Fn.batch_norm(h, None if training else P[name + ".norm.running_mean"],
                          None if training else P[name + ".norm.running_var"], P[name + ".norm.weight"],
                          P[name + ".norm.bias"], training, 0.0, 1e-5)
        h = torch.relu(h)
    h = Fn.conv1d(h, P["fc3.conv.weight"], P["fc3.conv.bias"])
    return h / (torch.norm(h, dim=1, keepdim=True) + eps)
