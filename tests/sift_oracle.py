"""An independent numpy restatement of the SIFT3D contract (include/usip_hip.h f-17): all-pairs squared distances
in sqdist's operation order, numpy.exp, a stable argsort for the 25 nearest, floor keys.  It shares no code with the library.
Besides the answer it measures, on the input, how far every decision sits from its threshold (four margins) and the bound on
the error of a DoG value that the tests hold the twin to."""
import numpy as np

NEAREST = 25
U = 1.1e-16
OFFSET = 1 << 20


def terrain(seed, n, side, amp):
    """a noisy height field: six Gaussian bumps over a square, f32 [n,3]"""
    g = np.random.default_rng(seed)
    xy = g.uniform(-side/2, side/2, (n, 2))
    c = g.uniform(-side/2, side/2, (6, 2)); h = g.uniform(-amp, amp, 6); w = g.uniform(1.0, 2.5, 6)
    z = sum(h[k]*np.exp(-((xy-c[k])**2).sum(1)/(2*w[k]**2)) for k in range(6)) + 0.01*g.standard_normal(n)
    return np.concatenate((xy, z[:, None]), 1).astype(np.float32)


# name -> (terrain arguments, parameters); what a numpy prototype of the contract saw on them with field z: the rows of the
# octave clouds, the keypoints per octave, the largest member count of a query
INPUTS = {
    "A": ((0, 2000, 24, 1.5), dict(min_scale=0.5, n_octaves=2, n_scales_per_octave=3, min_contrast=0.02)),
    "B": ((1, 3000, 30, 2.0), dict(min_scale=0.5, n_octaves=3, n_scales_per_octave=3, min_contrast=0.02)),
    "C": ((3, 600, 12, 1.0), dict(min_scale=0.5, n_octaves=2, n_scales_per_octave=2, min_contrast=0.02)),
}
CLOUDS = {"A": (1471, 756), "B": (2379, 1324, 456), "C": (390, 155)}
KEYPOINTS = {"A": (6, 10), "B": (9, 7, 3), "C": (2, 4)}
MEMBERS = {"A": 250, "B": 326}


def cloud_of(name):
    """pc f32 [3,n]"""
    return np.ascontiguousarray(terrain(*INPUTS[name][0]).T)


def reflectance(pc):
    """a supplied field: the reflectance-like column 0.5 + 0.3 sin(x), f32 [n]"""
    return (0.5 + 0.3 * np.sin(pc[0].astype(np.float64))).astype(np.float32)


def voxel(pc, field, leaf):
    """pc f32 [3,n], field an axis 0..2 or f32 [n] -> (cloud f32 [3,m], field f32 [m]) in ascending key"""
    p = pc.astype(np.float64)
    cell = np.floor(p / np.float64(leaf))
    keep = np.isfinite(cell).all(0) & (cell >= -OFFSET).all(0) & (cell < OFFSET).all(0)
    rows = np.flatnonzero(keep)
    c = cell[:, rows].astype(np.int64) + OFFSET
    key = (c[0] << 42) | (c[1] << 21) | c[2]
    order = rows[np.argsort(key, kind="stable")]
    key = np.sort(key, kind="stable")
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(key)]
    out = np.zeros((3, len(starts)), np.float32)
    fld = np.zeros(len(starts), np.float32)
    supplied = not isinstance(field, (int, np.integer))
    for r, (a, b) in enumerate(zip(starts, ends)):
        s = np.zeros(3, np.float64)
        sf = np.float64(0.0)
        for j in order[a:b]:                                            # ascending input index, one addition at a time
            s = s + p[:, j]
            if supplied:
                sf = sf + np.float64(field[j])
        out[:, r] = (s / np.float64(b - a)).astype(np.float32)
        fld[r] = np.float32(sf / np.float64(b - a)) if supplied else out[field, r]
    return out, fld


def sqdist_all(pc):
    """d2 f64 [n,n] in sqdist's order: (dx dx + dy dy) + dz dz"""
    p = pc.astype(np.float64)
    dx, dy, dz = (p[a][:, None] - p[a][None, :] for a in range(3))
    return (dx * dx + dy * dy) + dz * dz


def sigmas(base, k):
    return np.float64(base) * np.power(np.float64(2.0), (np.arange(k + 3, dtype=np.float64) - 1.0) / np.float64(k))


def octave(cloud, fld, base, k, min_contrast, exp_error):
    """One octave cloud of at least 25 rows -> dict: dog f64 [S-1,n], idx [n,25], mask, scale_index, the margins, the bound"""
    n = cloud.shape[1]
    sig = sigmas(base, k)
    S = len(sig)
    d2 = sqdist_all(cloud)
    f = fld.astype(np.float64)
    G = np.zeros((S, n))
    m_max, rel = 0, np.inf
    for s in range(S):
        s2 = sig[s] * sig[s]
        t = 9.0 * s2
        member = d2 < t
        w = np.where(member, np.exp(-((0.5 * d2) / s2)), 0.0)
        G[s] = (w * f[None, :]).sum(1) / w.sum(1)
        m_max = max(m_max, int(member.sum(1).max()))
        rel = min(rel, float((np.abs(d2 - t) / t).min()))
    dog = G[1:] - G[:-1]
    order = np.argsort(d2, axis=1, kind="stable")
    idx = order[:, :NEAREST]
    ranked = np.take_along_axis(d2, order[:, :NEAREST + 1], 1)
    gap = float(((ranked[:, NEAREST] - ranked[:, NEAREST - 1]) / ranked[:, NEAREST]).min()) if n > NEAREST else np.inf
    near = dog[:, idx]                                                  # [S-1, n, 25]
    mn, mx = near.min(2), near.max(2)
    mask = np.zeros(n, bool)
    scale = np.zeros(n, np.int32)
    contrast, tie = np.inf, np.inf
    for s in range(S - 3, 0, -1):
        v = dog[s]
        low = (v == mn[s]) & (v < mn[s - 1]) & (v < mn[s + 1])
        high = (v == mx[s]) & (v > mx[s - 1]) & (v > mx[s + 1])
        hit = (np.abs(v) >= min_contrast) & (low | high)
        mask |= hit
        scale[hit] = s
        contrast = min(contrast, float(np.abs(np.abs(v) - min_contrast).min()))
        diff = np.abs(near[s - 1:s + 2] - v[None, :, None])             # every value v could be compared with
        tie = min(tie, float(diff[diff > 0].min()))
    F = float(np.abs(f).max())
    bound = 2.0 * (2.0 * (exp_error + (m_max + 2) * U) * F)             # |dG| <= 2 (E + (m + 2) u) F, a DoG entry twice that
    return dict(cloud=cloud, field=fld, dog=dog, idx=idx.astype(np.int32), mask=mask, scale=scale, sigma=sig, m_max=m_max, F=F,
                bound=bound, d2_margin=rel, gap_margin=gap, contrast_margin=contrast, tie_margin=tie,
                dog_max=float(np.abs(dog).max()))


def sift(pc, field=2, min_scale=0.5, n_octaves=4, n_scales_per_octave=8, min_contrast=0.1, exp_error=0.0):
    """pc f32 [3,n] -> the list of octave dicts; the octaves end at the first cloud with fewer than 25 rows, whose dict holds
    only the cloud and its field"""
    out = []
    cloud, fld = pc, field
    for o in range(n_octaves):
        base = min_scale * 2.0 ** o
        cloud, fld = voxel(cloud, field if isinstance(field, (int, np.integer)) else fld, base)
        if cloud.shape[1] < NEAREST:
            out.append(dict(cloud=cloud, field=fld, mask=np.zeros(cloud.shape[1], bool)))
            break
        out.append(octave(cloud, fld, base, n_scales_per_octave, min_contrast, exp_error))
    return out
