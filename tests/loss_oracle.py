"""Plain references of the loss tail (csrc/nearest.hip, csrc/chamfer.hip) and the inputs their tests share.  numpy and
torch on the CPU only, integer or float64 arithmetic; independent of the library (usip_amd is not imported here).

Three references of the nearest-neighbour reduction, each with its own reach:
  nearest_exact_lattice  inputs on a lattice: squared distances are exact integers, so value AND first index are defined
                         without any summation order; the kernels must give these bits for every C.
  nearest_torch          C = 3, any input: torch.min over oracle.detector.pairwise_norm, the oracle the 3-D kernel is held to
                         bit for bit.
  nearest_f64            any C, any input: float64 distances; the kernel is held to bounds derived from its arithmetic.

Every bound below counts roundings of 2^-24 relative (U); none of them comes from a run.

Each lattice builder ASSERTS the property it exists for (enough queries whose minimum is attained by two or more
candidates), so that an edit of its parameters cannot quietly turn it into an easy input."""
import numpy as np
import torch

from oracle import detector as od

U = 2.0 ** -24                 # one fp32 rounding, relative
TIE_SHARE = 1.0 / 3.0          # least share of queries with a tied minimum in a lattice fixture


# ----------------------------------------------------------------------------------------------- the chunking rule
def chunk_plan(B, Ma, Nb):
    """-> (chunks, chunk length) of usip_nearest_f32's launch: a restatement of usip_nearest_workspace and of the
    launcher's rounding of the chunk to 64 candidates (csrc/nearest.hip); (1, Nb) when one launch does it.  The CPU test
    holds the chunk count to the library's own answer; the GPU tests place their candidates by the chunk length."""
    groups = B * ((Ma + 15) // 16)
    chunks = 1
    while groups * chunks < 1024 and Nb // (chunks * 2) >= 1024:
        chunks *= 2
    if chunks == 1:
        return 1, Nb
    return chunks, ((Nb + chunks - 1) // chunks + 63) // 64 * 64


# ----------------------------------------------------------------------------------------------- nearest: references
def _lattice_ints(a, b):
    """the common power-of-two step of a and b -> (int64 a, int64 b, k) with x = int * 2^-k exactly"""
    for k in range(0, 32):
        sa, sb = np.asarray(a, np.float64) * 2.0 ** k, np.asarray(b, np.float64) * 2.0 ** k
        if np.array_equal(sa, np.rint(sa)) and np.array_equal(sb, np.rint(sb)):
            return sa.astype(np.int64), sb.astype(np.int64), k
    raise AssertionError("the inputs are not on a power-of-two lattice")


def nearest_exact_lattice(a, b):
    """a [B,C,Ma], b [B,C,Nb] float32 on a lattice -> (d f32 [B,Ma], first arg-min i32 [B,Ma], tied bool [B,Ma]).
    Squared distances in int64 (asserted to fit 24 bits, so every partial sum of the kernels' FMA chain is exact in
    fp32), the value as numpy's correctly rounded float32 sqrt of the exact square, the index as the first arg-min of the
    integers; tied = the minimum is attained by two candidates or more."""
    a, b = np.asarray(a), np.asarray(b)
    ia, ib, k = _lattice_ints(a, b)
    B, C, Ma = ia.shape
    d = np.empty((B, Ma), np.float32)
    arg = np.empty((B, Ma), np.int32)
    tied = np.empty((B, Ma), bool)
    for bi in range(B):
        s = np.zeros((Ma, ib.shape[2]), np.int64)
        for c in range(C):
            df = ia[bi, c][:, None] - ib[bi, c][None, :]
            s += df * df
        assert int(s.max()) < 1 << 24, "squared distances leave fp32's exact integers"
        m = s.min(axis=1)
        arg[bi] = np.argmin(s, axis=1)
        tied[bi] = (s == m[:, None]).sum(axis=1) >= 2
        d[bi] = np.sqrt((m.astype(np.float64) * 4.0 ** -k).astype(np.float32))
    return d, arg, tied


def nearest_torch(a, b):
    """a [B,3,Ma], b [B,3,Nb] float32 -> (d f32 [B,Ma], arg i32 [B,Ma]) = torch.min(pairwise_norm(a, b), dim=2), one
    cloud at a time (the B x 3 x Ma x Nb difference of the whole batch is 800 MB at the largest shape; the norm over the
    three coordinates of one pair does not depend on how many clouds are formed together -- the CPU test checks it)."""
    return _nearest_torch(a, b)[:2]


def _nearest_torch(a, b):
    """nearest_torch and, per query, whether exactly one candidate attains the minimum distance"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    d, arg, single = [], [], []
    for bi in range(a.shape[0]):
        n = od.pairwise_norm(a[bi:bi + 1], b[bi:bi + 1])
        v, j = torch.min(n, dim=2)
        d.append(v)
        arg.append(j)
        single.append((n == v.unsqueeze(2)).sum(dim=2) == 1)
    return torch.cat(d).numpy(), torch.cat(arg).numpy().astype(np.int32), torch.cat(single).numpy()


def nearest_f64(a, b):
    """a [B,C,Ma], b [B,C,Nb] -> float64 distances [B,Ma,Nb] (minimum and arg-minimum are the caller's: the index
    assertion needs the distance of the candidate the kernel picked)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.zeros((a.shape[0], a.shape[2], b.shape[2]))
    for c in range(a.shape[1]):
        s += (a[:, c, :, None] - b[:, c, None, :]) ** 2
    return np.sqrt(s)


def nearest_nd_bounds(C):
    """(value, index) bounds of nearest_nd against nearest_f64, relative.  The squared distance is an FMA chain of C
    non-negative terms: each difference is rounded once (2 U on its square) and each FMA once, (C + 2) U in all; the
    square root halves it and rounds once more: |d - d64| <= (C/2 + 2) U d64.  A candidate the kernel prefers to the true
    minimum is at most two such errors above it: d64[got] <= min d64 (1 + (C + 4) U)."""
    return (C / 2.0 + 2.0) * U, (C + 4.0) * U


def nearest_backward_f64(a, b, arg, gd):
    """-> (ga f64 [B,C,Ma], gb f64 [B,C,Nb], n i64 [B,Nb], S f64 [B,Nb]): ga = gd (a - b[arg]) / |a - b[arg]|, exactly zero
    at zero distance; gb = - the sum of ga over the queries of every partner; n = the number of those queries and
    S = the sum of their |gd|.
    Bounds: |ga - ref| <= (C/2 + 6) U |gd_i| (one subtraction, the distance's own (C/2 + 2) U, one division, one product;
    every component of the unit vector is at most 1); |gb - ref| <= (n_j + C/2 + 6) U S_j (a sequential fp32 sum of n_j
    terms is the worst order of any)."""
    a, b, gd = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(gd, np.float64)
    arg = np.asarray(arg, np.int64)
    B, C, Ma = a.shape
    Nb = b.shape[2]
    sel = np.take_along_axis(b, np.broadcast_to(arg[:, None, :], (B, C, Ma)), axis=2)
    diff = a - sel
    dist = np.sqrt((diff ** 2).sum(axis=1))
    unit = np.where(dist[:, None, :] > 0, diff / np.where(dist > 0, dist, 1.0)[:, None, :], 0.0)
    ga = gd[:, None, :] * unit
    gb = np.zeros((B, C, Nb))
    n = np.zeros((B, Nb), np.int64)
    S = np.zeros((B, Nb))
    for bi in range(B):
        for c in range(C):
            np.subtract.at(gb[bi, c], arg[bi], ga[bi, c])
        np.add.at(n[bi], arg[bi], 1)
        np.add.at(S[bi], arg[bi], np.abs(gd[bi]))
    return ga, gb, n, S


def nearest_backward_bounds(C, gd, n, S):
    """-> (bound on ga [B,1,Ma], bound on gb [B,1,Nb]), absolute"""
    gd = np.abs(np.asarray(gd, np.float64))
    return (C / 2.0 + 6.0) * U * gd[:, None, :], ((n + C / 2.0 + 6.0) * U * S)[:, None, :]


# ----------------------------------------------------------------------------------------------- chamfer: reference
def chamfer_f64(a, J, c, I, ss, sd, gloss):
    """The three outputs and four gradients of the probabilistic chamfer loss (models/losses.py:82-99) by float64
    autograd, the loss weighted by `gloss` in the backward, and the magnitudes the bounds are made of.  -> dict:
      loss, pure, weighted        floats
      da, dc, dss, dsd            f64 arrays
      loss_mag                    mean|log s_f| + mean(a / s_f) + mean|log s_b| + mean(c / s_b): what the loss sums, signs off
      n_ss, H_ss, n_sd, H_sd      per target of the gathered sigma: the number of its sources, and the sum over them and
                                  its own term of the MAGNITUDE |gloss| / count / 2 (1/s + d/s^2), not of the cancelling
                                  difference 1/s - d/s^2 the gradient is
    Bounds (U = 2^-24): loss within 8 U loss_mag (the sums run in double on the device: what is left is logf, the
    division and the addition per element, and three roundings of the result); pure and weighted within 8 U |value|;
    da, dc within 4 U |ref| per element (scale, s, 1/s, their product); dss, dsd within (n_t + 8) U H_t."""
    J, I = torch.as_tensor(np.asarray(J)).long(), torch.as_tensor(np.asarray(I)).long()
    A, C, SS, SD = (torch.as_tensor(np.asarray(t)).double().requires_grad_(True) for t in (a, c, ss, sd))
    g = float(gloss)
    B, M = A.shape
    N = C.shape[1]
    sf = (SS + torch.gather(SD, 1, J)) / 2
    sb = (SD + torch.gather(SS, 1, I)) / 2
    loss = (torch.log(sf) + A / sf).mean() + (torch.log(sb) + C / sb).mean()
    pure = A.mean() + C.mean()
    wf, wb = (1 / sf) / (1 / sf).mean(), (1 / sb) / (1 / sb).mean()
    weighted = (wf * A).mean() + (wb * C).mean()
    (g * loss).backward()
    with torch.no_grad():
        mag = (torch.log(sf).abs().mean() + (A / sf).mean() + torch.log(sb).abs().mean() + (C / sb).mean()).item()
        hf = (abs(g) / (B * M) / 2 * (1 / sf + A / sf ** 2)).numpy()          # [B,M], lands on sd[J] and on ss itself
        hb = (abs(g) / (B * N) / 2 * (1 / sb + C / sb ** 2)).numpy()          # [B,N], lands on ss[I] and on sd itself
    H_sd, H_ss = hb.copy(), hf.copy()
    n_sd, n_ss = np.zeros((B, N), np.int64), np.zeros((B, M), np.int64)
    Jn, In = J.numpy(), I.numpy()
    for bi in range(B):
        np.add.at(H_sd[bi], Jn[bi], hf[bi])
        np.add.at(n_sd[bi], Jn[bi], 1)
        np.add.at(H_ss[bi], In[bi], hb[bi])
        np.add.at(n_ss[bi], In[bi], 1)
    return dict(loss=loss.item(), pure=pure.item(), weighted=weighted.item(), loss_mag=mag,
                da=A.grad.numpy(), dc=C.grad.numpy(), dss=SS.grad.numpy(), dsd=SD.grad.numpy(),
                n_ss=n_ss, H_ss=H_ss, n_sd=n_sd, H_sd=H_sd)


def chamfer_module_f64(src, dst, ss, sd, J, I, gloss=1.0):
    """ChamferLoss_Brute (models/losses.py:59-99) in float64 with the arg-minima GIVEN (the comparison at equal
    decisions): distances to the selected partners, the sigma arithmetic, and autograd's gradients of gloss * loss
    -> dict(loss, pure, weighted, gsrc, gdst, gss, gsd)"""
    J, I = torch.as_tensor(np.asarray(J)).long(), torch.as_tensor(np.asarray(I)).long()
    S, D, SS, SD = (torch.as_tensor(np.asarray(t)).double().requires_grad_(True) for t in (src, dst, ss, sd))
    a = torch.norm(S - torch.gather(D, 2, J.unsqueeze(1).expand(-1, 3, -1)), dim=1)
    c = torch.norm(D - torch.gather(S, 2, I.unsqueeze(1).expand(-1, 3, -1)), dim=1)
    sf = (SS + torch.gather(SD, 1, J)) / 2
    sb = (SD + torch.gather(SS, 1, I)) / 2
    loss = (torch.log(sf) + a / sf).mean() + (torch.log(sb) + c / sb).mean()
    pure = a.mean() + c.mean()
    weighted = ((1 / sf) / (1 / sf).mean() * a).mean() + ((1 / sb) / (1 / sb).mean() * c).mean()
    (float(gloss) * loss).backward()
    return dict(loss=loss.item(), pure=pure.item(), weighted=weighted.item(), gsrc=S.grad.numpy(), gdst=D.grad.numpy(),
                gss=SS.grad.numpy(), gsd=SD.grad.numpy())


def single_side_f64(kp, pc, arg, gd):
    """SingleSideChamferLoss_Brute (models/losses.py:125-143) in float64 with the arg-minimum given
    -> (d f64 [B,M], d/dkp of sum(gd * d) f64 [B,3,M])"""
    ga, _, _, _ = nearest_backward_f64(kp, pc, arg, gd)
    kp, pc = np.asarray(kp, np.float64), np.asarray(pc, np.float64)
    sel = np.take_along_axis(pc, np.broadcast_to(np.asarray(arg, np.int64)[:, None, :], kp.shape), axis=2)
    return np.sqrt(((kp - sel) ** 2).sum(axis=1)), ga


# ----------------------------------------------------------------------------------------------- builders
def _plant_duplicates(rng, b):
    """every candidate of the second half of a random order becomes a copy of one of the first half: the minimum of
    (almost) every query is then attained twice, at indices that fall into other lanes and other chunks"""
    Nb = b.shape[2]
    for bi in range(b.shape[0]):
        p = rng.permutation(Nb)
        h = Nb // 2
        b[bi][:, p[h:2 * h]] = b[bi][:, p[:h]]
    return b


def _assert_tied(a, b):
    if b.shape[2] >= 2:
        share = float(nearest_exact_lattice(a[:1], b[:1])[2].mean())
        assert share >= TIE_SHARE, "only %.2f of the queries have a tied minimum" % share


def cloud_random(seed, B, Ma, Nb):
    """two unrelated normal clouds, float32 [B,3,Ma] and [B,3,Nb]"""
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (B, 3, Ma)).astype(np.float32), rng.normal(0, 1, (B, 3, Nb)).astype(np.float32)


def cloud_random_rolled(seed, B, Ma, Nb, base=8):
    """-> (a, b, d, arg): B clouds that all differ, with nearest_torch's answer for each at the cost of `base` of them
    (torch.norm over B x Ma x Nb pairs takes 0.2 s per 10^6 on a CPU core).  Cloud bi is cloud bi % base with its queries
    permuted and its candidates rolled by a shift of its own; a pair's distance depends on the pair alone, so where the
    minimum distance of a query is attained by ONE candidate (asserted) the answer moves with the permutation and the
    shift: d[perm], (arg[perm] + shift) % Nb.  The CPU test compares this with nearest_torch run directly."""
    a0, b0 = cloud_random(seed, min(base, B), Ma, Nb)
    d0, j0, single = _nearest_torch(a0, b0)
    assert single.all(), "a tied minimum distance: the rolled answer is not defined by the base cloud's"
    rng = np.random.default_rng(seed + 1)
    a, b = np.empty((B, 3, Ma), np.float32), np.empty((B, 3, Nb), np.float32)
    d, arg = np.empty((B, Ma), np.float32), np.empty((B, Ma), np.int32)
    for bi in range(B):
        k = bi % a0.shape[0]
        perm = rng.permutation(Ma) if bi >= base else np.arange(Ma)
        shift = int(rng.integers(1, max(Nb, 2))) if bi >= base else 0
        a[bi], b[bi] = a0[k][:, perm], np.roll(b0[k], shift, axis=1)
        d[bi], arg[bi] = d0[k][perm], (j0[k][perm] + shift) % Nb
    return a, b, d, arg


def cloud_lattice(seed, B, Ma, Nb):
    """coordinates k/2 on [-4, 4]^3 (17^3 = 4913 sites; fewer sites per axis for few candidates), duplicates planted"""
    rng = np.random.default_rng(seed)
    side = int(np.clip(round((Nb / 2.0) ** (1.0 / 3.0)), 1, 8))
    a = (rng.integers(-side, side + 1, (B, 3, Ma)) / 2.0).astype(np.float32)
    b = _plant_duplicates(rng, (rng.integers(-side, side + 1, (B, 3, Nb)) / 2.0).astype(np.float32))
    _assert_tied(a, b)
    return a, b


def desc_lattice(seed, B, C, Ma, Nb):
    """descriptor entries in {-2..2} (in {-1, 0, 1} from C = 33 on: fewer distinct sums), duplicates planted"""
    rng = np.random.default_rng(seed)
    top = 2 if C < 33 else 1
    a = rng.integers(-top, top + 1, (B, C, Ma)).astype(np.float32)
    b = _plant_duplicates(rng, rng.integers(-top, top + 1, (B, C, Nb)).astype(np.float32))
    _assert_tied(a, b)
    return a, b


def desc_unit(seed, B, C, Ma, Nb):
    """unit-norm random descriptors, as the descriptor network's output is"""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(0, 1, (B, C, Ma)), rng.normal(0, 1, (B, C, Nb))
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return a.astype(np.float32), b.astype(np.float32)


CHAMFER_PATTERNS = ("random", "identity", "all_to_one", "first40")


def chamfer_inputs(seed, B, M, N, pattern, tiny_sigma=False):
    """-> (a f32 [B,M], J i32 [B,M], c f32 [B,N], I i32 [B,N], ss f32 [B,M], sd f32 [B,N]).  Sigmas uniform in
    [0.05, 1.5] and distances in [0, 1); tiny_sigma: every sigma at the lower bound 1e-3 and distances up to 100."""
    rng = np.random.default_rng(seed)
    top = 100.0 if tiny_sigma else 1.0
    a, c = rng.uniform(0, top, (B, M)).astype(np.float32), rng.uniform(0, top, (B, N)).astype(np.float32)
    if pattern == "random":
        J, I = rng.integers(0, N, (B, M)), rng.integers(0, M, (B, N))
    elif pattern == "identity":
        J, I = np.broadcast_to(np.arange(M) % N, (B, M)), np.broadcast_to(np.arange(N) % M, (B, N))
    elif pattern == "all_to_one":
        J, I = np.zeros((B, M)), np.full((B, N), M - 1)
    elif pattern == "first40":
        J, I = rng.integers(0, min(40, N), (B, M)), rng.integers(0, M, (B, N))
    else:
        raise ValueError(pattern)
    if tiny_sigma:
        ss, sd = np.full((B, M), 1e-3, np.float32), np.full((B, N), 1e-3, np.float32)
    else:
        ss, sd = rng.uniform(0.05, 1.5, (B, M)).astype(np.float32), rng.uniform(0.05, 1.5, (B, N)).astype(np.float32)
    return a, np.ascontiguousarray(J, np.int32), c, np.ascontiguousarray(I, np.int32), ss, sd
