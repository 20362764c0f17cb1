"""An independent restatement of the CGF triplet loss (include/usip_hip.h, f-22) for the tests: numpy, no code shared with the
library.

  select        float32 decisions from the keypoints and the uniforms, with numpy's first-arg-max / first-arg-min as the
                lowest-j tie rule
  loss          float64 loss, active share, saved distances and coefficients from the selection (math.fsum-free plain
                numpy float64: the tests compare at the bars of the number formats, and exactly on exact operands)
  backward      d_anc and d_pos by an ordered python loop
  philox_draws  the uniforms the library draws without explicit ones, by a Philox4x64-10 written on python integers
  dense_torch   the reference's forward (models/losses.py:240-314) restated densely in torch double from recorded draws, for
                autograd
"""
import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------- selection (float32)
def distances(anc_kp, pos_kp):
    """-> d f32 [B,M,M]: sqrt((dx dx + dy dy) + dz dz), every operation a float32 one"""
    a, p = np.asarray(anc_kp, F), np.asarray(pos_kp, F)
    dx = a[:, 0, :, None] - p[:, 0, None, :]
    dy = a[:, 1, :, None] - p[:, 1, None, :]
    dz = a[:, 2, :, None] - p[:, 2, None, :]
    return np.sqrt((dx * dx + dy * dy) + dz * dz, dtype=F)


def select(anc_kp, pos_kp, radius, u1, u2, u3):
    """-> (sel i32 [B,M,3], has u8 [B,M], take_far u8 [B,M])"""
    d = distances(anc_kp, pos_kp)
    r = F(radius)
    pos, out = d <= r, d > r
    j_pos = np.argmax(np.where(pos, np.asarray(u1, F), F(0)), axis=2)
    j_far = np.argmin(d + np.where(pos, F(1000), F(0)), axis=2)        # a float32 sum
    j_out = np.argmax(np.where(out, np.asarray(u2, F), F(0)), axis=2)
    sel = np.stack([j_pos, j_far, j_out], axis=2).astype(np.int32)
    return sel, pos.any(axis=2).astype(np.uint8), (np.asarray(u3, F) < F(0.5)).astype(np.uint8)


def negatives(sel, take_far):
    return np.where(take_far != 0, sel[:, :, 1], sel[:, :, 2])


# ---------------------------------------------------------------------------------------------------- loss (float64)
def descriptor_distance(a, p):
    """a, p f32 [C] -> the float64 distance in the contract's order: 64 strided partial sums, the binary tree, one sqrt"""
    sq = (a.astype(np.float64) - p.astype(np.float64)) ** 2
    part = [0.0] * 64
    for c in range(len(sq)):
        part[c % 64] += sq[c]
    s = 32
    while s:
        for l in range(s):
            part[l] += part[l + s]
        s //= 2
    return float(np.sqrt(np.float64(part[0])))


def ordered_weight_sum(raw):
    part = [0.0] * 256
    for i in range(len(raw)):
        part[i % 256] += float(raw[i])
    s = 128
    while s:
        for l in range(s):
            part[l] += part[l + s]
        s //= 2
    return part[0]


def loss(anc_desc, pos_desc, anc_sigma, sel, has, take_far, gamma, sigma_max):
    """-> dict(loss f32 [B,M], active f32 [B], dist f64 [B,M,2], coef f64 [B,M])"""
    B, C, M = anc_desc.shape
    jn = negatives(sel, take_far)
    dist = np.zeros((B, M, 2))
    coef = np.zeros((B, M))
    out = np.zeros((B, M), F)
    active = np.zeros((B,), F)
    for b in range(B):
        for i in range(M):
            dist[b, i, 0] = descriptor_distance(anc_desc[b, :, i], pos_desc[b, :, sel[b, i, 0]])
            dist[b, i, 1] = descriptor_distance(anc_desc[b, :, i], pos_desc[b, :, jn[b, i]])
        n1 = int(has[b].astype(np.int64).sum()) + 1
        before = np.where(has[b] != 0, (dist[b, :, 0] - dist[b, :, 1]) + float(gamma), 0.0)
        active[b] = F(float((before > 1e-5).sum()) / float(n1))
        raw = np.maximum(float(sigma_max) - anc_sigma[b].astype(np.float64), 0.0)
        mean = ordered_weight_sum(raw) / float(M)
        w = raw / mean if mean > 0.0 else np.zeros(M)
        coef[b] = np.where(before > 0.0, (w * float(M)) / float(n1), 0.0)
        out[b] = np.where(before > 0.0, coef[b] * before, 0.0).astype(F)
    return dict(loss=out, active=active, dist=dist, coef=coef)


def backward(anc_desc, pos_desc, sel, take_far, dist, coef, grad_loss):
    """-> (d_anc, d_pos) f32 [B,C,M]: d_pos adds its anchors in ascending order, the positive term before the negative"""
    B, C, M = anc_desc.shape
    jn = negatives(sel, take_far)
    a, p = anc_desc.astype(np.float64), pos_desc.astype(np.float64)
    d_anc = np.zeros((B, C, M))
    d_pos = np.zeros((B, C, M))

    def unit(v, dd):
        return v / dd if dd > 0.0 else np.zeros_like(v)

    for b in range(B):
        for i in range(M):
            g = float(grad_loss[b, i]) * coef[b, i]
            jp, jq = sel[b, i, 0], jn[b, i]
            up, un = unit(a[b, :, i] - p[b, :, jp], dist[b, i, 0]), unit(a[b, :, i] - p[b, :, jq], dist[b, i, 1])
            d_anc[b, :, i] = g * (up - un)
            d_pos[b, :, jp] -= g * up
            d_pos[b, :, jq] += g * un
    return d_anc.astype(F), d_pos.astype(F)


# ---------------------------------------------------------------------------------------------------- Philox on python integers
_M64 = (1 << 64) - 1
_KEY_WORD = int.from_bytes(b"cgf_loss", "big")
_TAG = 27


def philox4x64_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0 = (k0 + 0x9E3779B97F4A7C15) & _M64
            k1 = (k1 + 0xBB67AE8584CAA73B) & _M64
        p0, p1 = 0xD2E7470EE14C6C93 * c0, 0xCA5A826395121157 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & _M64, (p0 >> 64) ^ c3 ^ k1, p0 & _M64
    return c0, c1, c2, c3


def philox_draws(seed, step, elem, M):
    """the uniforms of global batch element `elem`: (u1 f32 [M,M], u2 f32 [M,M], u3 f32 [M])"""
    u1, u2, u3 = np.zeros((M, M), F), np.zeros((M, M), F), np.zeros((M,), F)
    key = (seed & _M64, _KEY_WORD)
    for i in range(M):
        u3[i] = F(philox4x64_10((i, (_TAG << 8) | 1, elem, step), key)[0] >> 40) * F(2.0 ** -24)
        for j in range(M):
            w = philox4x64_10(((i << 16) | j, _TAG << 8, elem, step), key)
            u1[i, j] = F(w[0] >> 40) * F(2.0 ** -24)
            u2[i, j] = F(w[1] >> 40) * F(2.0 ** -24)
    return u1, u2, u3


# ---------------------------------------------------------------------------------------------------- the reference's dense form
def dense_torch(anc_kp, anc_desc, pos_kp, pos_desc, anc_sigma, radius, gamma, sigma_max, u1, u2, u3):
    """models/losses.py:240-314 on torch tensors with the three recorded uniform arrays in place of torch.rand.  Keypoints
    stay float32 (the decisions are float32 ones); descriptors and sigmas may be double leaves -> (loss [B,M], active [B])."""
    import torch
    B, M = anc_kp.shape[0], anc_kp.shape[2]
    ddiff = torch.norm(anc_desc.unsqueeze(3) - pos_desc.unsqueeze(2), dim=1)
    kdiff = torch.from_numpy(distances(anc_kp.numpy(), pos_kp.numpy()))
    pos_mask = kdiff <= np.float32(radius)
    has = pos_mask.any(dim=2).to(ddiff.dtype)
    nearby = torch.max(pos_mask.float() * u1, dim=2, keepdim=True)[1]
    d_pos = torch.gather(ddiff, 2, nearby).squeeze(2)
    far = torch.min(kdiff + pos_mask.float() * 1000, dim=2, keepdim=True)[1]
    d_far = torch.gather(ddiff, 2, far).squeeze(2)
    outside = torch.max(u2 * (kdiff > np.float32(radius)).float(), dim=2, keepdim=True)[1]
    d_out = torch.gather(ddiff, 2, outside).squeeze(2)
    pick = (u3 < 0.5).to(ddiff.dtype)
    d_neg = pick * d_far + (1 - pick) * d_out
    scaling = (M / (has.sum(dim=1) + 1)).detach()
    before = (d_pos - d_neg + gamma) * has
    active = (before > 1e-5).to(ddiff.dtype).sum(dim=1) / (has.sum(dim=1) + 1)
    w = torch.clamp(sigma_max - anc_sigma, min=0)
    w = (w / w.mean(dim=1, keepdim=True)).detach()
    return w * torch.clamp(before, min=0) * scaling.unsqueeze(1), active
