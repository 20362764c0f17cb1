"""An independent restatement of the ISS contract (include/usip_hip.h f-11) in numpy float64: an all-pairs
distance matrix, numpy.linalg.eigvalsh, numpy's own summation order.  It shares nothing with the product.

Besides its results it returns two MARGINS, because a comparison with it is meaningful only where no decision sits on a
threshold: `gate` = the smallest |e2/e1 - gamma_21| and |e3/e2 - gamma_32| over the points that reach the gates, `tie` = the
smallest relative saliency difference between a salient point and a distinct neighbour within the non-maximum radius.  A test
first asserts both exceed MARGIN -- a condition on its input, not on the product."""
import numpy as np

MARGIN = 1e-9
# (seed, n, h): slab clouds x, z ~ U(-h, h), y ~ N(0, 1); radii 2 / 2, gamma 0.975, min 5.  Checked on a CPU with this file
# alone: gate margins >= 2.3e-5, tie margins >= 3.6e-8, and these keypoint counts
INPUTS = ((0, 257, 8.0), (1, 1000, 12.0), (2, 3000, 20.0), (3, 3000, 3.0))
KEYPOINTS = {(0, 257, 8.0): 15, (1, 1000, 12.0): 33, (2, 3000, 20.0): 92, (3, 3000, 3.0): 2}


def slab(seed: int, n: int, h: float) -> np.ndarray:
    """float32 [3,n]"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-h, h, n), rng.normal(0, 1, n), rng.uniform(-h, h, n)]).astype(np.float32)


def iss(pc, salient_radius=2.0, non_max_radius=2.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """pc [3,n] -> dict(mask bool [n], saliency [n], neighbours [n], trace [n], gate, tie)."""
    p = np.asarray(pc, dtype=np.float64).T                             # [n,3]
    n = len(p)
    d = p[None, :, :] - p[:, None, :]                                  # d[i,j] = p_j - p_i
    d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
    near = d2 < salient_radius * salient_radius
    neighbours = near.sum(1)
    C = np.einsum("ij,ija,ijb->iab", near.astype(np.float64), d, d)
    e = np.linalg.eigvalsh(C)                                          # ascending
    e3, e2, e1 = e[:, 0], e[:, 1], e[:, 2]
    reach = neighbours >= min_neighbors
    with np.errstate(divide="ignore", invalid="ignore"):
        r21, r32 = e2 / e1, e3 / e2
        ok = reach & np.isfinite(e).all(1) & (e3 >= 0) & (r21 < gamma_21) & (r32 < gamma_32)
    saliency = np.where(ok, e3, 0.0)
    gates = np.concatenate((np.abs(r21[reach] - gamma_21), np.abs(r32[reach] - gamma_32)))
    gates = gates[np.isfinite(gates)]
    close = d2 < non_max_radius * non_max_radius
    larger = (close & (saliency[None, :] > saliency[:, None])).any(1)
    mask = (saliency > 0) & (close.sum(1) >= min_neighbors) & ~larger
    pair = close & ~np.eye(n, dtype=bool) & (saliency > 0)[:, None]
    si, sj = np.broadcast_to(saliency[:, None], (n, n))[pair], np.broadcast_to(saliency[None, :], (n, n))[pair]
    rel = np.abs(si - sj) / np.maximum(si, sj)
    return dict(mask=mask, saliency=saliency, neighbours=neighbours.astype(np.int32), trace=np.trace(C, axis1=1, axis2=2),
                gate=float(gates.min()) if gates.size else np.inf, tie=float(rel.min()) if rel.size else np.inf)
