"""Indoor fragment registration on the device: the number the reference reports for its indoor models,
registration recall / precision on the Redwood / 3DMatch fragment benchmark (evaluation/matlab/eval_indoor/3dmatch:
runFragmentRegistration.m -> clusterCallback.m -> register2Fragments.m -> writeLog.m -> evaluate.m ->
mrEvaluateRegistrationMy.m).

  match_descriptors_topk   pdist2(b, a, 'euclidean', 'smallest', k) on ragged batches
  match_union              union([i, nn12(i, :)], [nn21(q, :), q], 'rows')
  fragment_registration    ransacfitRt on up to 10240 correspondences (threshold 0.2, ransac.m's default 30000 trials)
  fgr_registration         Fast Global Registration (eval_indoor/fgr/register2FragmentsFGR.m; Zhou, Park, Koltun 2016) on the
                           mutual nearest descriptors: tuple test, 64 Gauss-Newton steps (csrc/fgr.hip)
  information_matrix       the 6 x 6 sum of A'A over the inliers' fragment-1 keypoints
  overlap_ratio            ratioAligned: the share of each full fragment with a point of the other closer than 0.2 m
  RefineBank / icp_refine  writeLogReconputeAlign.m: both fragments voxel-averaged at 0.04 m, the estimate refined by trimmed
                           point-to-point ICP (pcregrigid's InlierRatio 0.3), the share of moved points within 0.05 m and
                           the second gate, `> 0.15` (csrc/icp.hip); metric "point_to_plane", on a bank built
                           with normals, is pcregrigid's 'pointToPlane' (csrc/icp_plane_math.h)
  optimize                 split_txt_compute_G.m and the robust pose-graph optimisation behind it: the dense information of
                           every pair under its refined pose, the loop closures the graph does not support pruned, recall
                           and precision after pruning (usip_amd/posegraph.py, csrc/posegraph.hip)
  *_cpu                    the same on numpy arrays over the library's host twins (csrc/fragments_cpu.cpp; RANSAC:
                           evaluation.ransac_*_cpu with the limit at 10240)
  transformation_error     mrComputeTransformationError with the file's own dcm2quat
  evaluate_log             mrEvaluateRegistrationMy: recall, precision, mean inlier number and ratio (host numpy)
  read_* / write_*         gt.log (mrLoadLog), gt.info (mrLoadInfo), <scene>.log (writeLog.m / mrLoadLogMy) and the
                           per-pair i-j.rt.txt of clusterCallback.m
  FragmentEvaluator        detector -> NMS / top-k -> descriptor per fragment, cached beside the fragment's full cloud;
                           evaluate() runs every pair on the device, reads the host once and scores

RANSAC draws are f-6's (usip_amd/evaluation.py): the reference's algorithm on Philox draws keyed by (seed, pair id, trial).
"""
from collections import namedtuple
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, inference, ops, prepare
from .evaluation import _np, _p, ransac_select_cpu, ransac_trials_cpu, select_keypoints_device

FragmentResult = namedtuple("FragmentResult",
                            "Rt inliers inlier_mask trialcount valid delta_t delta_deg chosen counts inlier_ratio")
LogEntry = namedtuple("LogEntry", "info trans")                               # gt.log: (i, j, n), 4 x 4
InfoEntry = namedtuple("InfoEntry", "info mat")                               # gt.info: (i, j, n), 6 x 6
FgrResult = namedtuple("FgrResult", "Rt inliers inlier_mask valid delta_t delta_deg counts inlier_ratio mutual rows row_count "
                                    "trials_walked")
ResultEntry = namedtuple("ResultEntry", "info trans inlier_num inlier_ratio information")
PairFile = namedtuple("PairFile", "fragment1 fragment2 inlier_num inlier_ratio ratio_aligned trans information")

INLIER_THRESHOLD, MAX_TRIALS, OVERLAP_RADIUS, K_MATCH = 0.2, 30000, 0.2, 5
GATE_ALIGNED, GATE_INLIER_RATIO = 0.23, 0.025                                # writeLog.m
GATE_REFINED, REFINE_LEAF, REFINE_RADIUS, REFINE_INLIER_RATIO = 0.15, 0.04, 0.05, 0.3      # writeLogReconputeAlign.m
REFINE_ITERATIONS, REFINE_TOLERANCE = 20, (0.01, 0.009)                      # pcregrigid's documented defaults
IcpResult = namedtuple("IcpResult", "Rt iterations converged rmse hits ratio")
REFINE_METRICS, NORMALS_K = ops.ICP_METRICS, 9                                # f-28: pcregrigid's 'Metric'; f-7's neighbours
REFINE_KEYS = ("refined_Rt", "refine_iterations", "refine_converged", "refined_ratio_aligned", "refined_hits", "gate_refined")


# ------------------------------------------------------------------------------------------------ device
def match_descriptors_topk(anc_desc, pos_desc, anc_count, pos_count, k: int = K_MATCH):
    """anc_desc f32 [P,C,Ma], pos_desc f32 [P,C,Mp], counts i32 [P] -> (idx i32 [P,Ma,k], valid i32 [P]): for every anchor
    descriptor its k nearest positive descriptors, ascending, the lower index on ties; valid = min(k, pos_count) columns
    hold data."""
    _, idx, valid = ops.knn_nd_counted(anc_desc, pos_desc, anc_count, pos_count, k)
    return idx, valid


def match_union(nn12, nn21, count1, count2):
    """-> (pairs i32 [P,Cmax,2], count i32 [P]): the unique rows (i, q) of both lists, sorted."""
    return ops.match_union(nn12, nn21, count1, count2)


def _finish(o, count, counts, eye):
    valid = o["valid"]
    ok = valid.reshape(-1, 1, 1) != 0
    Rt = (torch.where if isinstance(valid, torch.Tensor) else np.where)(ok, o["Rt"], eye)
    ratio = o["inliers"] / (torch.clamp(count, min=1) if isinstance(count, torch.Tensor) else np.maximum(count, 1))
    return FragmentResult(Rt, o["inliers"], o["inlier_mask"], o["trialcount"], valid, None, None, o["chosen"], counts, ratio)


def fragment_registration(x1, x2, count, threshold: float = INLIER_THRESHOLD, max_trials: int = MAX_TRIALS, seed: int = 0,
                          pair_ids=None, triplets=None) -> FragmentResult:
    """x1 = R x2 + t from matched coordinates x1, x2 f32 [P,3,Nmax] with count i32 [P], Nmax <= 10240.  The fields of
    evaluation.RegistrationResult plus inlier_ratio = inliers / count (0 without correspondences).  An invalid pair (fewer
    than 3 correspondences or inliers) gets [I | 0], 0 inliers and an empty mask, as register2Fragments.m's catch branch.
    Device tensors, no host synchronisation."""
    T = int(max_trials) + 1 if triplets is None else int(triplets.shape[1])
    counts, _, _ = ops.ransac_trials_large(x1, x2, count, T, threshold, seed, pair_ids, triplets)
    o = ops.ransac_select_large(x1, x2, count, counts, min(int(max_trials), T - 1), threshold, seed, pair_ids, triplets)
    eye = torch.eye(3, 4, dtype=torch.float64, device=x1.device)
    return _finish(o, count.to(torch.float64), counts, eye)


def _finish_fgr(t, o, lib_np):
    count = t["mutual_count"]
    ratio = o["inliers"] / (np.maximum(count, 1) if lib_np else torch.clamp(count, min=1).to(torch.float64))
    return FgrResult(o["Rt"], o["inliers"], o["inlier_mask"], o["valid"], None, None, count, ratio, t["mutual"], t["rows"],
                     t["row_count"], t["trials_walked"])


def fgr_registration(kp1, kp2, n1, n2, nn12, nn21, threshold: float = INLIER_THRESHOLD, seed: int = 0, pair_ids=None,
                     triples=None) -> FgrResult:
    """x1 = R x2 + t by Fast Global Registration from the keypoints kp1, kp2 f32 [P,3,M] (M <= 1024) with counts n1, n2 i32
    [P] and the nearest descriptors nn12, nn21 i32 [P,M] of match_descriptors_topk(k = 1) in both directions.  The fields of
    fragment_registration without trialcount and chosen, plus mutual i32 [P,M,2] (the mutual nearest rows, `counts` of them
    per pair), rows i32 [P,3000] with row_count (the tuple test's rows, indices into mutual) and trials_walked.  inlier_mask
    u8 [P,M] and inlier_ratio = inliers / counts are over the mutual rows.  An invalid pair (no scale, fewer than 10 rows, a
    failed solve) gets [I | 0], 0 inliers and an empty mask.  Device tensors, no host synchronisation."""
    t = ops.fgr_tuples(kp1, kp2, n1, n2, nn12, nn21, seed, pair_ids, triples)
    o = ops.fgr_optimize(kp1, kp2, t["mutual"], t["mutual_count"], t["norm"], t["rows"], t["row_count"], threshold)
    return _finish_fgr(t, o, False)


def information_matrix(x1, inlier_mask):
    """x1 f32 [P,3,Nmax] (the fragment-1 keypoint of every correspondence), inlier_mask u8 [P,Nmax] -> f64 [P,6,6]."""
    return ops.information(x1, inlier_mask)


def _pack(parts, device):
    """Fragments' rows [n,3] on the device -> the fields of a bank: lengths, offsets (host and device), rows in ONE buffer,
    every fragment's local row indices ascending along x, lmax."""
    lengths = [int(p.shape[0]) for p in parts]
    offsets_host = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return dict(lengths=lengths, offsets_host=offsets_host, rows=torch.cat(parts).contiguous(),
                offsets=torch.from_numpy(offsets_host).to(device),
                perm=torch.cat([torch.argsort(p[:, 0], stable=True).to(torch.int32) for p in parts]).contiguous(),
                lmax=max(max(lengths), 1))


def _rows3(c, device):
    c = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c)[:, :3], dtype=np.float32))
    return c.to(device, torch.float32)[:, :3]


class FragmentBank:
    """The fragments' full clouds in ONE float32 device buffer [rows, 3] with int64 offsets (CSR, as pairs.ScanBank holds
    scans), plus, per fragment, its local row indices ascending along x."""

    def __init__(self, clouds: Sequence, device):
        self.device = torch.device(device)
        parts = [_rows3(c, self.device) for c in clouds]
        if not parts:
            raise ValueError("%s: no fragments" % type(self).__name__)
        self.__dict__.update(_pack(parts, self.device))

    def host(self):
        return HostBank(self.rows.cpu().numpy(), self.offsets_host.copy(), self.perm.cpu().numpy(), self.lmax)


HostBank = namedtuple("HostBank", "rows offsets perm lmax")


def host_bank(clouds: Sequence) -> HostBank:
    parts = [np.ascontiguousarray(np.asarray(c)[:, :3], dtype=np.float32) for c in clouds]
    offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    perm = np.concatenate([np.argsort(p[:, 0], kind="stable").astype(np.int32) for p in parts])
    return HostBank(np.concatenate(parts), offsets, perm, max(max(p.shape[0] for p in parts), 1))


def moved_x_order(bank, frag2, Rt):
    """-> i32 [P,lmax]: every pair's fragment-2 rows ascending along their moved x, sorted on the device by the keys the
    library computes (stable; padding last).  Rt contiguous f64 [P,3,4]."""
    keys = ops.overlap_keys(bank.rows, bank.offsets, frag2, Rt, bank.lmax)
    return torch.argsort(keys, dim=1, stable=True).to(torch.int32)


def overlap_ratio(bank: FragmentBank, frag1, frag2, Rt, radius: float = OVERLAP_RADIUS):
    """frag1, frag2 i32 [P] (fragments of the bank), Rt f64 [P,3,4] moving fragment 2 into fragment 1's frame ->
    (ratio f64 [P,2], hits i32 [P,2]): register2Fragments.m's ratioAligned.  The moved fragment is sorted along x here,
    on the device, by the keys the library computes."""
    Rt = Rt.contiguous()
    return ops.overlap_ratio(bank.rows, bank.offsets, frag1, frag2, Rt, bank.perm, moved_x_order(bank, frag2, Rt), radius)


def chordal_tolerance(tol_r: float) -> float:
    """|R - R'|_F of two rotations tol_r radians apart, 2 sqrt(2) sin(tol_r / 2): the bound the library compares with."""
    return 2.0 * math.sqrt(2.0) * math.sin(0.5 * float(tol_r))


class RefineBank(FragmentBank):
    """The fragments' clouds voxel-averaged at `leaf` (pcdownsample 'gridAverage', f-7's kernels; positions only: a zero
    reflectance column and zero normals go in), in ONE float32 device buffer [rows, 3] with offsets and the x-order of every
    fragment, as FragmentBank holds the full clouds.  Built once per scene: every fragment's cell count is read from the
    device here, nothing is read after.

    normals=True (what the point-to-plane metric reads, f-28): the buffer is [rows, 6], the voxel-averaged positions and
    their unit normals -- per fragment f-7's 9 nearest neighbours (ops.scan_knn on the bank's own x-order) and ops.scan_normals
    of the DOWNSAMPLED rows, turned towards the fragment frame's origin, its float32 rounding.  A fragment of fewer than 10
    downsampled rows is below scan_knn's limit and gets zero normals: a pair that takes it as fragment 1 fails its first
    plane fit and keeps the pose it came with."""

    def __init__(self, clouds: Sequence, device, leaf: float = REFINE_LEAF, normals: bool = False):
        self.leaf, self.normals = float(leaf), bool(normals)
        if not self.leaf > 0.0:
            raise ValueError("RefineBank: leaf must be positive")
        FragmentBank.__init__(self, [self._downsample(_rows3(c, torch.device(device))) for c in clouds], device)
        if self.normals:
            self.rows = torch.cat((self.rows, self._normals()), 1).contiguous()

    def _normals(self):
        out = self.rows.new_zeros((self.rows.shape[0], 3))
        for lo, n in zip(self.offsets_host.tolist(), self.lengths):
            if n < NORMALS_K + 1:
                continue
            xyzi = torch.cat((self.rows[lo:lo + n], self.rows.new_zeros((n, 1))), 1).contiguous()
            idx = ops.scan_knn(xyzi, self.perm[lo:lo + n].contiguous(), NORMALS_K)
            out[lo:lo + n] = ops.scan_normals(xyzi, idx, (0.0, 0.0, 0.0))[1][:, :3]
        return out

    def _downsample(self, xyz):
        n = xyz.shape[0]
        if n == 0:
            return xyz.new_zeros((0, 3))
        pts = torch.cat((xyz, xyz.new_zeros((n, 1))), 1).contiguous()
        lo, hi = torch.aminmax(xyz, dim=0)
        keys = ops.scan_voxel_keys(pts, torch.cat((lo, hi)).contiguous(), self.leaf)
        skeys, order = torch.sort(keys, stable=True)
        _, counts = torch.unique_consecutive(skeys, return_counts=True)
        start = torch.zeros(counts.shape[0] + 1, dtype=torch.int32, device=pts.device)
        start[1:] = torch.cumsum(counts, 0)
        nrm = torch.zeros((n, 4), dtype=torch.float64, device=pts.device)
        return ops.scan_voxel_average(pts, nrm, order.to(torch.int32), start)[:, :3].contiguous()


def _refine_args(inlier_ratio, max_iterations, tolerance, align_radius):
    if len(tolerance) != 2:
        raise ValueError("icp_refine: tolerance is (translation, rotation in radians)")
    return float(inlier_ratio), int(max_iterations), float(tolerance[0]), chordal_tolerance(tolerance[1]), float(align_radius)


def icp_refine(bank: RefineBank, frag1, frag2, Rt, mask=None, inlier_ratio: float = REFINE_INLIER_RATIO,
               max_iterations: int = REFINE_ITERATIONS, tolerance=REFINE_TOLERANCE,
               align_radius: float = REFINE_RADIUS, want_cuts: bool = False, metric: str = "point_to_point",
               want_sums: bool = False) -> IcpResult:
    """writeLogReconputeAlign.m's refinement for a batch of pairs, on the device: frag1, frag2 i32 [P] into the bank, Rt f64
    [P,3,4] the estimate (fragment 2 into fragment 1), mask bool or u8 [P] (pairs with 0 are not refined: Rt stays, the rest
    is 0).  tolerance = (translation, rotation in radians) on the mean change of the last three iterations, pcregrigid's.
    -> IcpResult(Rt, iterations, converged, rmse, hits, ratio f64 [P,2] = hits over either fragment's downsampled length).
    Fragment 2's rows are sorted along their moved x here, by the keys the library computes.  No host synchronisation.
    want_cuts: -> (IcpResult, cut_d2 f64, cut_i i32 [P,max_iterations+1]), the trim's cut of every pass, the final pass last.
    metric "point_to_plane" (f-28; the bank built with normals=True, otherwise ValueError): every kept row is drawn towards
    the plane through its nearest row instead of towards the row; the trim, the stopping rule, the final pass and the
    fields are the same.  want_sums (that metric only): the tuple ends with fit_sums f64 [P,max_iterations,27]."""
    ir, it, tt, tc, ar = _refine_args(inlier_ratio, max_iterations, tolerance, align_radius)
    Rt = Rt.contiguous()
    m = None if mask is None else mask.to(torch.uint8).contiguous()
    o = ops.icp_refine(bank.rows, bank.offsets, bank.perm, frag1, frag2, Rt, bank.lmax, m, moved_x_order(bank, frag2, Rt),
                       ir, it, tt, tc, ar, want_cuts=want_cuts, metric=metric, want_sums=want_sums)
    res = IcpResult(o["Rt"], o["iterations"], o["converged"], o["rmse"], o["hits"], o["ratio"])
    extra = ((o["cut_d2"], o["cut_i"]) if want_cuts else ()) + ((o["fit_sums"],) if want_sums else ())
    return (res,) + extra if extra else res


def _refined(out, res: IcpResult):
    out.update(refined_Rt=res.Rt, refine_iterations=res.iterations, refine_converged=res.converged,
               refined_ratio_aligned=res.ratio, refined_hits=res.hits,
               gate_refined=(res.ratio[:, 0] > GATE_REFINED) & (out["inlier_ratio"] > GATE_INLIER_RATIO))
    return out


# ------------------------------------------------------------------------------------------------ host twins (numpy)
def match_descriptors_topk_cpu(anc_desc, pos_desc, anc_count, pos_count, k: int = K_MATCH, num_threads: int = 1,
                               want_dist: bool = False):
    a, b = _np(anc_desc, np.float32, "anc_desc"), _np(pos_desc, np.float32, "pos_desc")
    B, C, Ma = a.shape
    Nb = b.shape[2]
    ac, bc = _np(anc_count, np.int32, "anc_count", (B,)), _np(pos_count, np.int32, "pos_count", (B,))
    k = int(k)
    d, idx, valid = np.zeros((B, Ma, k), np.float32), np.zeros((B, Ma, k), np.int32), np.zeros(B, np.int32)
    _lib.check(_lib.lib().usip_knn_nd_counted_f32_cpu(_p(a), _p(b), _p(ac), _p(bc), k, _p(d), _p(idx), _p(valid), B, C, Ma,
                                                      Nb, int(num_threads)), "usip_knn_nd_counted_f32_cpu")
    return (idx, valid, d) if want_dist else (idx, valid)


def match_union_cpu(nn12, nn21, count1, count2):
    a, b = _np(nn12, np.int32, "nn12"), _np(nn21, np.int32, "nn21")
    P, Ma, k = a.shape
    Mp = b.shape[1]
    c1, c2 = _np(count1, np.int32, "count1", (P,)), _np(count2, np.int32, "count2", (P,))
    pairs, count = np.zeros((P, k * (Ma + Mp), 2), np.int32), np.zeros(P, np.int32)
    _lib.check(_lib.lib().usip_match_union_i32_cpu(_p(a), _p(b), _p(c1), _p(c2), P, Ma, Mp, k, _p(pairs), _p(count)),
               "usip_match_union_i32_cpu")
    return pairs, count


def ransac_trials_large_cpu(x1, x2, count, T: int, threshold: float = INLIER_THRESHOLD, seed: int = 0, pair_ids=None,
                            triplets=None, num_threads: int = 1):
    """evaluation.ransac_trials_cpu with Nmax <= 10240."""
    return ransac_trials_cpu(x1, x2, count, T, threshold, seed, pair_ids, triplets, num_threads, _nmax=ops.RANSAC_NMAX_LARGE)


def ransac_select_large_cpu(x1, x2, count, counts, max_trials: int, threshold: float = INLIER_THRESHOLD, seed: int = 0,
                            pair_ids=None, triplets=None) -> Dict[str, np.ndarray]:
    """evaluation.ransac_select_cpu with Nmax <= 10240."""
    return ransac_select_cpu(x1, x2, count, counts, max_trials, threshold, seed, pair_ids, triplets,
                             _nmax=ops.RANSAC_NMAX_LARGE)


def fragment_registration_cpu(x1, x2, count, threshold: float = INLIER_THRESHOLD, max_trials: int = MAX_TRIALS,
                              seed: int = 0, pair_ids=None, triplets=None, num_threads: int = 1) -> FragmentResult:
    T = int(max_trials) + 1 if triplets is None else int(np.shape(triplets)[1])
    counts, _, _ = ransac_trials_large_cpu(x1, x2, count, T, threshold, seed, pair_ids, triplets, num_threads)
    o = ransac_select_large_cpu(x1, x2, count, counts, min(int(max_trials), T - 1), threshold, seed, pair_ids, triplets)
    return _finish(o, np.asarray(count, np.float64), counts, np.eye(3, 4))


def fgr_tuples_cpu(kp1, kp2, n1, n2, nn12, nn21, seed: int = 0, pair_ids=None, triples=None, want_triples: int = 0,
                   num_threads: int = 1) -> Dict[str, np.ndarray]:
    """ops.fgr_tuples on numpy arrays over the host twin."""
    a, b = _np(kp1, np.float32, "kp1"), _np(kp2, np.float32, "kp2")
    if a.ndim != 3 or a.shape[1] != 3 or b.shape != a.shape:
        raise ValueError("expected kp1, kp2 [P,3,M]")
    P, _, M = a.shape
    if not (1 <= M <= ops.FGR_MMAX and P <= 65535):                        # the device entries' rule and error
        raise RuntimeError("fgr: M must be in 1..%d and P at most 65535 (got P = %d, M = %d)" % (ops.FGR_MMAX, P, M))
    c1, c2 = _np(n1, np.int32, "n1", (P,)), _np(n2, np.int32, "n2", (P,))
    f12 = _np(np.reshape(nn12, (P, -1)), np.int32, "nn12", (P, M))
    f21 = _np(np.reshape(nn21, (P, -1)), np.int32, "nn21", (P, M))
    ids = None if pair_ids is None else _np(pair_ids, np.int64, "pair_ids", (P,))
    tr = None if triples is None else _np(triples, np.int32, "triples")
    if tr is not None and (tr.ndim != 3 or tr.shape[0] != P or tr.shape[1] < 1 or tr.shape[2] != 3):
        raise ValueError("triples must be i32 [P,T,3]")
    out = {"mutual": np.zeros((P, M, 2), np.int32), "mutual_count": np.zeros(P, np.int32), "norm": np.zeros((P, 8)),
           "rows": np.zeros((P, ops.FGR_ROWS_MAX), np.int32), "row_count": np.zeros(P, np.int32),
           "trials_walked": np.zeros(P, np.int32),
           "triples": np.zeros((P, int(want_triples), 3), np.int32) if want_triples and tr is None else None}
    _lib.check(_lib.lib().usip_fgr_tuples_f32_cpu(
        _p(a), _p(b), _p(c1), _p(c2), _p(f12), _p(f21), P, M, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(ids), _p(tr),
        tr.shape[1] if tr is not None else 0, _p(out["mutual"]), _p(out["mutual_count"]), _p(out["norm"]), _p(out["rows"]),
        _p(out["row_count"]), _p(out["trials_walked"]), _p(out["triples"]), int(want_triples), int(num_threads)),
        "usip_fgr_tuples_f32_cpu")
    return out


def fgr_optimize_cpu(kp1, kp2, mutual, mutual_count, norm, rows, row_count, threshold: float = INLIER_THRESHOLD,
                     num_threads: int = 1) -> Dict[str, np.ndarray]:
    """ops.fgr_optimize on numpy arrays over the host twin."""
    a, b = _np(kp1, np.float32, "kp1"), _np(kp2, np.float32, "kp2")
    if a.ndim != 3 or a.shape[1] != 3 or b.shape != a.shape:
        raise ValueError("expected kp1, kp2 [P,3,M]")
    P, _, M = a.shape
    if not (1 <= M <= ops.FGR_MMAX and P <= 65535):
        raise RuntimeError("fgr: M must be in 1..%d and P at most 65535 (got P = %d, M = %d)" % (ops.FGR_MMAX, P, M))
    mu, mc = _np(mutual, np.int32, "mutual", (P, M, 2)), _np(mutual_count, np.int32, "mutual_count", (P,))
    nm, rw = _np(norm, np.float64, "norm", (P, 8)), _np(rows, np.int32, "rows", (P, ops.FGR_ROWS_MAX))
    rc = _np(row_count, np.int32, "row_count", (P,))
    out = {"Rt": np.zeros((P, 3, 4)), "valid": np.zeros(P, np.uint8), "inlier_mask": np.zeros((P, M), np.uint8),
           "inliers": np.zeros(P, np.int32)}
    _lib.check(_lib.lib().usip_fgr_optimize_f32_cpu(
        _p(a), _p(b), _p(mu), _p(mc), _p(nm), _p(rw), _p(rc), P, M, float(threshold), _p(out["Rt"]), _p(out["valid"]),
        _p(out["inlier_mask"]), _p(out["inliers"]), int(num_threads)), "usip_fgr_optimize_f32_cpu")
    return out


def fgr_registration_cpu(kp1, kp2, n1, n2, nn12, nn21, threshold: float = INLIER_THRESHOLD, seed: int = 0, pair_ids=None,
                         triples=None, num_threads: int = 1) -> FgrResult:
    t = fgr_tuples_cpu(kp1, kp2, n1, n2, nn12, nn21, seed, pair_ids, triples, 0, num_threads)
    o = fgr_optimize_cpu(kp1, kp2, t["mutual"], t["mutual_count"], t["norm"], t["rows"], t["row_count"], threshold,
                         num_threads)
    return _finish_fgr(t, o, True)


def information_matrix_cpu(x1, inlier_mask):
    x = _np(x1, np.float32, "x1")
    P, _, Nmax = x.shape
    m = _np(inlier_mask, np.uint8, "inlier_mask", (P, Nmax))
    info = np.zeros((P, 6, 6))
    _lib.check(_lib.lib().usip_information_f32_cpu(_p(x), _p(m), P, Nmax, _p(info)), "usip_information_f32_cpu")
    return info


def _host_bank_args(bank: HostBank):
    """-> (the C argument run rows, row_len, offsets, num_frags, total_rows of a HostBank, the arrays it points into: the
    caller keeps them until the call has returned)"""
    rows, offsets = _np(bank.rows, np.float32, "rows"), _np(bank.offsets, np.int64, "offsets")
    return (_p(rows), rows.shape[1], _p(offsets), offsets.shape[0] - 1, rows.shape[0]), (rows, offsets)


def overlap_ratio_cpu(bank: HostBank, frag1, frag2, Rt, radius: float = OVERLAP_RADIUS, prune: bool = True,
                      num_threads: int = 1):
    args, alive = _host_bank_args(bank)
    perm1 = _np(bank.perm, np.int32, "perm", (args[-1],))
    f2 = _np(frag2, np.int32, "frag2")
    P = f2.shape[0]
    f1, G = _np(frag1, np.int32, "frag1", (P,)), _np(Rt, np.float64, "Rt", (P, 3, 4))
    perm2 = moved_x_order_cpu(bank, f2, G)
    hits, ratio = np.zeros((P, 2), np.int32), np.zeros((P, 2))
    _lib.check(_lib.lib().usip_overlap_ratio_f32_cpu(*args, _p(f1), _p(f2), _p(G), _p(perm1), _p(perm2), P, int(bank.lmax),
                                                     float(radius), 1 if prune else 0, _p(hits), _p(ratio),
                                                     int(num_threads)), "usip_overlap_ratio_f32_cpu")
    return ratio, hits


def refine_bank_cpu(clouds: Sequence, leaf: float = REFINE_LEAF, normals: bool = False) -> HostBank:
    """RefineBank on the host: every cloud through the grid average's host twin -> HostBank of the downsampled rows [rows, 3];
    normals=True: [rows, 6], with the normals of prepare.knn_cpu / normals_cpu on the downsampled rows (zeros below 10 rows)."""
    parts = []
    for c in clouds:
        a = np.ascontiguousarray(np.asarray(c)[:, :3], dtype=np.float32)
        if a.shape[0]:
            xyzi = np.ascontiguousarray(np.concatenate((a, np.zeros((a.shape[0], 1), np.float32)), 1))
            a = np.ascontiguousarray(prepare.grid_cpu(xyzi, np.zeros((a.shape[0], 4)), float(leaf))[0][:, :3])
        parts.append(a)
    if not parts:
        raise ValueError("refine_bank_cpu: no fragments")
    bank = host_bank(parts)
    if not normals:
        return bank
    nrm = np.zeros((bank.rows.shape[0], 3), np.float32)
    for lo, a in zip(bank.offsets.tolist(), parts):
        if a.shape[0] >= NORMALS_K + 1:
            xyzi = np.ascontiguousarray(np.concatenate((a, np.zeros((a.shape[0], 1), np.float32)), 1))
            nrm[lo:lo + a.shape[0]] = prepare.normals_cpu(xyzi, None, NORMALS_K, (0.0, 0.0, 0.0))[2][:, :3]
    return bank._replace(rows=np.ascontiguousarray(np.concatenate((bank.rows, nrm), 1)))


def _icp_host(bank: HostBank, frag1, frag2, Rt, mask, order2):
    args, alive = _host_bank_args(bank)
    perm1 = _np(bank.perm, np.int32, "perm", (args[-1],))
    f2 = _np(frag2, np.int32, "frag2")
    P = f2.shape[0]
    if P > 65535:
        raise RuntimeError("icp: at most 65535 pairs per call (got %d)" % P)
    f1, G = _np(frag1, np.int32, "frag1", (P,)), _np(Rt, np.float64, "Rt", (P, 3, 4))
    L = int(bank.lmax)
    m = None if mask is None else _np(np.asarray(mask).astype(np.uint8), np.uint8, "mask", (P,))
    o2 = None if order2 is None else _np(order2, np.int32, "order2", (P, L))
    return args + (_p(perm1), _p(f1), _p(f2), _p(G), _p(m), _p(o2), P, L), alive + (perm1, f1, f2, G, m, o2)


def moved_x_order_cpu(bank: HostBank, frag2, Rt):
    """-> i32 [P,lmax]: every pair's fragment-2 rows ascending along their moved x (usip_overlap_keys_f32_cpu, stable)."""
    args, alive = _host_bank_args(bank)
    f2 = _np(frag2, np.int32, "frag2")
    P, L = f2.shape[0], int(bank.lmax)
    G = _np(Rt, np.float64, "Rt", (P, 3, 4))
    keys = np.zeros((P, L))
    _lib.check(_lib.lib().usip_overlap_keys_f32_cpu(*args, _p(f2), _p(G), P, L, _p(keys)), "usip_overlap_keys_f32_cpu")
    return np.ascontiguousarray(np.argsort(keys, axis=1, kind="stable").astype(np.int32))


def icp_nearest_cpu(bank: HostBank, frag1, frag2, Rt, mask=None, order2=None, num_threads: int = 1):
    """ops.icp_nearest on numpy arrays over the host twin (the loop over all rows) -> (idx i32 [P,lmax], d2 f64 [P,lmax])."""
    args, alive = _icp_host(bank, frag1, frag2, Rt, mask, order2)
    P, L = args[-2:]
    idx, d2 = np.zeros((P, L), np.int32), np.zeros((P, L))
    _lib.check(_lib.lib().usip_icp_nearest_f32_cpu(*args, _p(idx), _p(d2), int(num_threads)), "usip_icp_nearest_f32_cpu")
    return idx, d2


def icp_refine_cpu(bank: HostBank, frag1, frag2, Rt, mask=None, inlier_ratio: float = REFINE_INLIER_RATIO,
                   max_iterations: int = REFINE_ITERATIONS, tolerance=REFINE_TOLERANCE, align_radius: float = REFINE_RADIUS,
                   num_threads: int = 1, want_neighbours: bool = False, order2="moved_x", want_cuts: bool = False,
                   metric: str = "point_to_point", want_sums: bool = False):
    """icp_refine on numpy arrays over the host twin -> IcpResult; with want_neighbours also the final pass's (idx, d2); with
    want_cuts also (cut_d2 f64, cut_i i32) [P,max_iterations+1]: the trim's cut (d2*, i*) of every pass, the final pass last;
    with want_sums (metric "point_to_plane" only) also fit_sums f64 [P,max_iterations,27]."""
    if metric not in REFINE_METRICS:
        raise ValueError("icp: metric must be one of %s (got %r)" % (", ".join(REFINE_METRICS), metric))
    plane = metric == "point_to_plane"
    if want_sums and not plane:
        raise ValueError("icp: want_sums is the point_to_plane metric's")
    if plane and np.shape(bank.rows)[1] < 6:
        raise ValueError("icp: the point_to_plane metric needs a bank with normals, rows f32 [total,>=6] (got row_len %d)"
                         % np.shape(bank.rows)[1])
    ir, it, tt, tc, ar = _refine_args(inlier_ratio, max_iterations, tolerance, align_radius)
    if isinstance(order2, str):
        order2 = moved_x_order_cpu(bank, frag2, Rt)
    args, alive = _icp_host(bank, frag1, frag2, Rt, mask, order2)
    P, L = args[-2:]
    out = IcpResult(np.zeros((P, 3, 4)), np.zeros(P, np.int32), np.zeros(P, np.uint8), np.zeros(P), np.zeros(P, np.int32),
                    np.zeros((P, 2)))
    idx, d2 = (np.zeros((P, L), np.int32), np.zeros((P, L))) if want_neighbours else (None, None)
    cd, ci = (np.zeros((P, it + 1)), np.zeros((P, it + 1), np.int32)) if want_cuts else (None, None)
    sums = np.zeros((P, it, 27)) if want_sums else None
    name = "usip_icp_refine_plane_f32_cpu" if plane else "usip_icp_refine_f32_cpu"
    _lib.check(getattr(_lib.lib(), name)(
        *args, ir, it, tt, tc, ar, _p(out.Rt), _p(out.iterations), _p(out.converged), _p(out.rmse), _p(out.hits),
        _p(out.ratio), _p(cd), _p(ci), _p(idx), _p(d2), *((_p(sums),) if plane else ()), int(num_threads)), name)
    extra = ((idx, d2) if want_neighbours else ()) + ((cd, ci) if want_cuts else ()) + ((sums,) if want_sums else ())
    return (out,) + extra if extra else out


# ------------------------------------------------------------------------------------------------ the per-pair pipeline
# what _register_pairs runs over: the library's steps on device tensors, or on numpy arrays over the host twins
_Backend = namedtuple("_Backend", "match union gather ransac fgr information overlap refine dense points index")


def _dense(name):
    def call(*args):
        from . import posegraph
        return getattr(posegraph, name)(*args)
    return call


_DEVICE = _Backend(match_descriptors_topk, match_union,
                   lambda kp, rows: torch.gather(kp, 2, rows.long().unsqueeze(1).expand(-1, 3, -1)).contiguous(),
                   fragment_registration, fgr_registration, information_matrix, overlap_ratio, icp_refine,
                   _dense("dense_information"), lambda kp: kp, lambda frag: frag)


def _host(nt: int) -> _Backend:
    return _Backend(
        lambda a, b, na, nb, k: match_descriptors_topk_cpu(a, b, na, nb, k, nt), match_union_cpu,
        lambda kp, rows: np.ascontiguousarray(np.take_along_axis(kp, np.broadcast_to(rows[:, None, :],
                                                                                     (len(kp), 3, rows.shape[1])), 2)),
        lambda *a: fragment_registration_cpu(*a, None, nt), lambda *a: fgr_registration_cpu(*a, None, nt),
        information_matrix_cpu, lambda *a: overlap_ratio_cpu(*a, True, nt),
        lambda *a, **kw: icp_refine_cpu(*a, num_threads=nt, **kw), lambda *a: _dense("dense_information_cpu")(*a, nt),
        lambda kp: np.asarray(kp, np.float32), lambda frag: np.asarray(frag, np.int32))


def _register_pairs(be, name, kp1, desc1, n1, kp2, desc2, n2, bank, frag1, frag2, pair_ids, k, threshold, max_trials, radius,
                    seed, registrator, refine, refine_args, dense_radius, refine_metric):
    """register_pairs over the backend `be` (_DEVICE, or _host(num_threads))."""
    if registrator not in ("ransac", "fgr"):
        raise ValueError("registrator must be 'ransac' or 'fgr' (got %r)" % (registrator,))
    if dense_radius is not None and refine is None:
        raise ValueError("%s: dense_radius needs refine" % name)
    if refine_metric not in REFINE_METRICS:
        raise ValueError("%s: refine_metric must be one of %s (got %r)" % (name, ", ".join(REFINE_METRICS), refine_metric))
    k = 1 if registrator == "fgr" else k
    nn12, _ = be.match(desc1, desc2, n1, n2, k)
    nn21, _ = be.match(desc2, desc1, n2, n1, k)
    kp1, kp2 = be.points(kp1), be.points(kp2)
    if registrator == "fgr":
        reg = be.fgr(kp1, kp2, n1, n2, nn12, nn21, threshold, seed, pair_ids)
        x1 = be.gather(kp1, reg.mutual[:, :, 0])
        out = dict(Rt=reg.Rt, inliers=reg.inliers, inlier_ratio=reg.inlier_ratio, valid=reg.valid, matches=reg.counts,
                   row_count=reg.row_count, trials_walked=reg.trials_walked)
    else:
        pairs, count = be.union(nn12, nn21, n1, n2)
        x1, x2 = be.gather(kp1, pairs[:, :, 0]), be.gather(kp2, pairs[:, :, 1])
        reg = be.ransac(x1, x2, count, threshold, max_trials, seed, pair_ids)
        out = dict(Rt=reg.Rt, inliers=reg.inliers, inlier_ratio=reg.inlier_ratio, trialcount=reg.trialcount, valid=reg.valid,
                   chosen=reg.chosen, matches=count)
    frag1, frag2 = be.index(frag1), be.index(frag2)
    ratio, hits = be.overlap(bank, frag1, frag2, reg.Rt, radius)
    out.update(information=be.information(x1, reg.inlier_mask), ratio_aligned=ratio, overlap_hits=hits,
               gate=(ratio[:, 0] > GATE_ALIGNED) & (reg.inlier_ratio > GATE_INLIER_RATIO), frag1=frag1, frag2=frag2)
    if refine is not None:
        mask = (out["valid"] != 0) & (out["inlier_ratio"] > GATE_INLIER_RATIO)
        _refined(out, be.refine(refine, frag1, frag2, out["Rt"], mask, metric=refine_metric, **(refine_args or {})))
        if dense_radius is not None:
            out["dense_information"], out["dense_count"] = be.dense(refine, frag1, frag2, out["refined_Rt"], mask, dense_radius)
    return out


def register_pairs(kp1, desc1, n1, kp2, desc2, n2, bank: FragmentBank, frag1, frag2, pair_ids, k: int = K_MATCH,
                   threshold: float = INLIER_THRESHOLD, max_trials: int = MAX_TRIALS, radius: float = OVERLAP_RADIUS,
                   seed: int = 0, registrator: str = "ransac", refine: Optional[RefineBank] = None,
                   refine_args: Optional[Dict] = None, dense_radius: Optional[float] = None,
                   refine_metric: str = "point_to_point") -> Dict[str, torch.Tensor]:
    """register2Fragments.m for a batch of pairs, on the device: kp f32 [P,3,M], desc f32 [P,D,M], n i32 [P] of either
    fragment; frag1, frag2 i32 [P] into the bank; pair_ids i64 [P] key the draws.  No host synchronisation.

    registrator "fgr" is register2FragmentsFGR.m instead: the nearest descriptor in both directions (k = 1; `k` and
    `max_trials` are not used) -> fgr_registration -> the information matrix over the mutual inliers -> the same overlap
    walk and gate.  The reference's FGR wrapper hard-codes ratioAligned = 0.8 and inlierRatio = 0.99 and so writes every
    pair to its log; here the gate sees the measured values, as for RANSAC.  Its keys: RANSAC's without trialcount and
    chosen, plus row_count and trials_walked; matches counts the mutual rows.

    refine: the scene's RefineBank (its fragments in the bank's order) adds writeLogReconputeAlign.m to either registrator:
    icp_refine(refine, frag1, frag2, Rt, mask = valid & inlier_ratio > 0.025, **refine_args) and the keys refined_Rt,
    refine_iterations, refine_converged, refined_ratio_aligned, refined_hits and gate_refined = refined ratio(1) > 0.15 &
    inlier_ratio > 0.025.  A pair outside the mask fails that gate whatever ICP would find.  Every other key is unchanged.
    refine_metric "point_to_plane" (f-28) refines under the plane metric instead, on a bank that carries normals
    (RefineBank(..., normals=True)); the keys are the same under either metric.

    dense_radius (with refine): split_txt_compute_G.m's computeInformation 'point' under refined_Rt, over the same mask:
    the keys dense_information f64 [P,6,6] and dense_count i32 [P] (posegraph.dense_information)."""
    return _register_pairs(_DEVICE, "register_pairs", kp1, desc1, n1, kp2, desc2, n2, bank, frag1, frag2, pair_ids, k,
                           threshold, max_trials, radius, seed, registrator, refine, refine_args, dense_radius, refine_metric)


def register_pairs_cpu(kp1, desc1, n1, kp2, desc2, n2, bank: HostBank, frag1, frag2, pair_ids, k: int = K_MATCH,
                       threshold: float = INLIER_THRESHOLD, max_trials: int = MAX_TRIALS, radius: float = OVERLAP_RADIUS,
                       seed: int = 0, num_threads: int = 1, registrator: str = "ransac", refine: Optional[HostBank] = None,
                       refine_args: Optional[Dict] = None, dense_radius: Optional[float] = None,
                       refine_metric: str = "point_to_point") -> Dict[str, np.ndarray]:
    """register_pairs assembled from the host twins, on numpy arrays; refine: the HostBank of the downsampled fragments
    (refine_bank_cpu, or RefineBank.host(); with normals for refine_metric "point_to_plane")."""
    return _register_pairs(_host(int(num_threads)), "register_pairs_cpu", kp1, desc1, n1, kp2, desc2, n2, bank, frag1, frag2,
                           pair_ids, k, threshold, max_trials, radius, seed, registrator, refine, refine_args, dense_radius,
                           refine_metric)


# ------------------------------------------------------------------------------------------------ the score
def dcm2quat(R):
    """ElasticReconstruction's own dcm2quat (mrEvaluateRegistrationMy.m), float64; NaN / inf when the trace is -1."""
    R = np.asarray(R, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q0 = 0.5 * np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
        return np.array([q0, -(R[2, 1] - R[1, 2]) / (4 * q0), -(R[0, 2] - R[2, 0]) / (4 * q0),
                         -(R[1, 0] - R[0, 1]) / (4 * q0)])


def transformation_error(gt_trans, result_trans, gt_info) -> float:
    """mrComputeTransformationError(gt_trans^-1 * result_trans, gt_info): er = [t; -q(2:4)], er' info er / info(1, 1)."""
    trans = np.linalg.inv(np.asarray(gt_trans, np.float64)) @ np.asarray(result_trans, np.float64)
    info = np.asarray(gt_info, np.float64)
    er = np.concatenate((trans[:3, 3], -dcm2quat(trans[:3, :3])[1:]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(er @ info @ er / info[0, 0])


def evaluate_log(result: Sequence, gt: Sequence, gt_info: Sequence, err2: float = 0.04) -> Dict:
    """mrEvaluateRegistrationMy: result = ResultEntry rows, gt = LogEntry rows, gt_info = InfoEntry rows (same order as
    gt).  Only pairs with j - i > 1 count; a result pair absent from gt is a false positive; a NaN error is not good."""
    if not len(gt):
        raise ValueError("evaluate_log: the ground truth is empty")
    num = int(gt[0].info[2])
    mask, gt_num = {}, 0
    for k, g in enumerate(gt):
        if g.info[1] - g.info[0] > 1:
            mask[int(g.info[0]) + int(g.info[1]) * num] = k
            gt_num += 1
    rs_num = good = bad = false_pos = 0
    errors, inlier_num, inlier_ratio = [], [], []
    for r in result:
        if r.info[1] - r.info[0] > 1:
            rs_num += 1
            k = mask.get(int(r.info[0]) + int(r.info[1]) * num)
            if k is None:
                false_pos += 1
                continue
            p = transformation_error(gt[k].trans, r.trans, gt_info[k].mat)
            errors.append(p)
            if p <= err2:
                good += 1
                inlier_num.append(r.inlier_num)
                inlier_ratio.append(r.inlier_ratio)
            else:
                bad += 1
    nan = float("nan")
    return {"recall": good / gt_num if gt_num else nan, "precision": good / rs_num if rs_num else nan,
            "inlier_num_mean": float(np.mean(inlier_num)) if inlier_num else nan,
            "inlier_ratio_mean": float(np.mean(inlier_ratio)) if inlier_ratio else nan,
            "good": good, "bad": bad, "false_pos": false_pos, "gt_num": gt_num, "rs_num": rs_num,
            "errors": np.asarray(errors, np.float64)}


# ------------------------------------------------------------------------------------------------ files
def _tokens(path):
    with open(path) as f:
        return f.read().split()


def _blocks(path, floats):
    tok, out, at = _tokens(path), [], 0
    while at + 3 <= len(tok):
        info = tuple(int(v) for v in tok[at:at + 3])
        vals = [float(v) for v in tok[at + 3:at + 3 + floats]]
        if len(vals) < floats:
            break
        out.append((info, vals))
        at += 3 + floats
    return out


def read_log(path) -> List[LogEntry]:
    """mrLoadLog: blocks of `i j n` and a 4 x 4 matrix, row by row."""
    return [LogEntry(i, np.array(v).reshape(4, 4)) for i, v in _blocks(path, 16)]


def write_log(path, entries: Sequence):
    with open(path, "w") as f:
        for e in entries:
            f.write("%d\t%d\t%d\n" % tuple(e.info))
            for row in np.asarray(e.trans, np.float64).reshape(4, 4):
                f.write("%.8e\t%.8e\t%.8e\t%.8e\n" % tuple(row))


def read_info(path) -> List[InfoEntry]:
    """mrLoadInfo: blocks of `i j n` and a 6 x 6 matrix, row by row."""
    return [InfoEntry(i, np.array(v).reshape(6, 6)) for i, v in _blocks(path, 36)]


def write_info(path, entries: Sequence):
    with open(path, "w") as f:
        for e in entries:
            f.write("%d\t%d\t%d\n" % tuple(e.info))
            for row in np.asarray(e.mat, np.float64).reshape(6, 6):
                f.write(" ".join("%.8f" % v for v in row) + "\n")


def read_result_log(path) -> List[ResultEntry]:
    """mrLoadLogMy: `i j n`, the 4 x 4 estimate row by row, `inliers ratio`, the 6 x 6 information column by column."""
    out = []
    for info, v in _blocks(path, 16 + 2 + 36):
        out.append(ResultEntry(info, np.array(v[:16]).reshape(4, 4), int(round(v[16])), v[17],
                               np.array(v[18:]).reshape(6, 6).T))
    return out


def write_result_log(path, entries: Sequence):
    """writeLog.m's block per pair that passed the gate."""
    with open(path, "w") as f:
        for e in entries:
            f.write("%d\t %d\t %d\t\n" % tuple(e.info))
            for row in np.asarray(e.trans, np.float64).reshape(4, 4):
                f.write("%.10f\t%.10f\t%.10f\t%.10f\n" % tuple(row))
            f.write("%d\t%f\n" % (int(e.inlier_num), float(e.inlier_ratio)))
            for col in np.asarray(e.information, np.float64).reshape(6, 6).T:
                f.write("%.10f\t%.10f\t%.10f\t%.10f\t%.10f\t%.10f\n" % tuple(col))


def write_pair_file(path, p: PairFile):
    """clusterCallback.m:32-34, the i-j.rt.txt of one pair."""
    with open(path, "w") as f:
        f.write("%d\t %d\t\n%d\t %15.8e\t %15.8e\t %15.8e\t\n" % (p.fragment1, p.fragment2, p.inlier_num, p.inlier_ratio,
                                                                  p.ratio_aligned[0], p.ratio_aligned[1]))
        for row in np.asarray(p.trans, np.float64).reshape(4, 4):
            f.write("%15.8e\t %15.8e\t %15.8e\t %15.8e\t\n" % tuple(row))
        for col in np.asarray(p.information, np.float64).reshape(6, 6).T:
            f.write("%15.8e\t %15.8e\t %15.8e\t %15.8e\t %15.8e\t %15.8e\t\n" % tuple(col))


def read_pair_file(path) -> PairFile:
    """What writeLog.m's dlmread calls take from an i-j.rt.txt."""
    v = _tokens(path)
    if len(v) < 2 + 4 + 16 + 36:
        raise ValueError("%s: not a pair file" % path)
    x = [float(t) for t in v[2:]]
    return PairFile(int(v[0]), int(v[1]), int(round(x[0])), x[1], (x[2], x[3]), np.array(x[4:20]).reshape(4, 4),
                    np.array(x[20:56]).reshape(6, 6).T)


def read_descriptors_bin(path, dim: int):
    """Utils.load_descriptors: float32 rows [x y z descriptor(dim)] -> (xyz [M,3], desc [M,dim])."""
    a = np.fromfile(path, dtype=np.float32).reshape(-1, 3 + int(dim))
    return a[:, :3].copy(), a[:, 3:].copy()


def write_descriptors_bin(path, xyz, desc):
    np.concatenate((np.asarray(xyz, np.float32), np.asarray(desc, np.float32)), 1).astype(np.float32).tofile(path)


def to4x4(Rt):
    return np.concatenate((np.asarray(Rt, np.float64).reshape(3, 4), [[0.0, 0.0, 0.0, 1.0]]))


def result_entries(per_pair: Dict[str, np.ndarray], fragment_ids: Sequence[int], num_fragments: int, gate: str = "gate",
                   transform: str = "Rt") -> List[ResultEntry]:
    """writeLog.m: the pairs that pass `ratioAligned(1) > 0.23 && inlierRatio > 0.025`, in the order they were run.
    gate "gate_refined", the recomputed `> 0.15`, is writeLogReconputeAlign.m, which still writes the unrefined estimate
    (transform "Rt"); transform "refined_Rt" writes the refined one."""
    out = []
    for p in np.nonzero(per_pair[gate])[0]:
        out.append(ResultEntry((int(fragment_ids[per_pair["frag1"][p]]), int(fragment_ids[per_pair["frag2"][p]]),
                                int(num_fragments)), to4x4(per_pair[transform][p]), int(per_pair["inliers"][p]),
                               float(per_pair["inlier_ratio"][p]), per_pair["information"][p]))
    return out


# ------------------------------------------------------------------------------------------------ the evaluator
class FragmentEvaluator:
    """Scores a detector + descriptor pair on scene fragments the way the reference's MATLAB does, without leaving the
    device: the indoor sibling of evaluation.RegistrationEvaluator.

    add_fragment(id, pc, sn, node, cloud) runs detector -> NMS / top-k -> descriptor on one fragment ([1,3,N], [1,Cs,N],
    [1,3,M] device tensors) and caches keypoints, descriptors and count beside the fragment's full cloud ([rows, >= 3]);
    add_fragment_result(id, xyz, desc, cloud) takes precomputed [xyz, descriptor] rows, what the .bin files hold.  Ids
    are the fragments' integer indices in the scene.  evaluate(pairs, gt, gt_info) runs the pairs (default: all i < j) in
    batches through register_pairs, reads the host once, applies writeLog.m's gate and scores with evaluate_log.

    optimize (needs refine): split_txt_compute_G.m and the optimisation behind it.  Every pair's dense information is taken
    under refined_Rt; the pairs that pass the log's gate are the graph's edges, with the log's transform (log_transform);
    the graph is built and optimised on the device before the one read (posegraph.prune_pairs).  optimize_args: tau2,
    prune, iterations1, iterations2 (include/usip_hip.h f-14), fill ("gt": a missing odometry pair comes from gt.log and
    gt.info, the default when evaluate() is given them; "estimate": from the pair's ungated estimate; None), transform
    ("edge" or "graph": what the refined log's entries hold), radius.  summarize() then also returns loop_recall,
    loop_precision, loops_in, loops_kept, and per pair dense_information, dense_count, loop_weight, loop_kept, loop_Rt.

    refine_metric "point_to_plane" (with refine): the refinement runs under the plane metric (f-28) and refine_bank() builds
    the downsampled fragments' normals; the second gate, the refined log and the graph read the same keys as before."""

    def __init__(self, detector, descriptor, opt, device, nms_radius: float = 0.1, top: int = 512, k: int = K_MATCH,
                 inlier_threshold: float = INLIER_THRESHOLD, max_trials: int = MAX_TRIALS,
                 overlap_radius: float = OVERLAP_RADIUS, seed: int = 0, batch_pairs: int = 32, registrator: str = "ransac",
                 refine: bool = False, refine_leaf: float = REFINE_LEAF, refine_args: Optional[Dict] = None,
                 log_transform: str = "estimate", optimize: bool = False, optimize_args: Optional[Dict] = None,
                 refine_metric: str = "point_to_point"):
        if refine_metric not in REFINE_METRICS:
            raise ValueError("refine_metric must be one of %s (got %r)" % (", ".join(REFINE_METRICS), refine_metric))
        self.refine_metric = refine_metric
        if log_transform not in ("estimate", "refined"):
            raise ValueError("log_transform must be 'estimate' or 'refined' (got %r)" % (log_transform,))
        if log_transform == "refined" and not refine:
            raise ValueError("FragmentEvaluator: log_transform 'refined' needs refine=True")
        self.refine, self.refine_leaf, self.refine_args = bool(refine), float(refine_leaf), dict(refine_args or {})
        self.log_transform = log_transform
        self._refine_bank = None
        if optimize and not refine:
            raise ValueError("FragmentEvaluator: optimize=True needs refine=True (the dense information is taken under the "
                             "refined pose)")
        self.optimize, self.optimize_args = bool(optimize), dict(optimize_args or {})
        if self.optimize:
            from . import posegraph
            posegraph.split_optimize_args(self.optimize_args)              # an unknown key is refused here
        if registrator not in ("ransac", "fgr"):
            raise ValueError("registrator must be 'ransac' or 'fgr' (got %r)" % (registrator,))
        if registrator == "fgr" and int(top) > ops.FGR_MMAX:
            raise ValueError("FragmentEvaluator: registrator 'fgr' takes at most %d keypoints per fragment" % ops.FGR_MMAX)
        self.registrator = registrator
        self.detector, self.descriptor, self.opt = detector, descriptor, opt
        self.device = torch.device(device)
        self.nms_radius, self.top, self.k = float(nms_radius), int(top), int(k)
        self.inlier_threshold, self.max_trials = float(inlier_threshold), int(max_trials)
        self.overlap_radius, self.seed, self.batch_pairs = float(overlap_radius), int(seed), int(batch_pairs)
        self.fragments = {}
        self._bank = None

    def _store(self, fragment_id, kp, desc, count, cloud):
        width = self.top
        if kp.shape[1] > width:
            raise ValueError("FragmentEvaluator: fragment %s has %d keypoints, top is %d" % (fragment_id, kp.shape[1], width))
        if kp.shape[1] < width:                                    # one width for batching; padding is never read
            kp = torch.cat((kp, kp.new_zeros(3, width - kp.shape[1])), 1)
            desc = torch.cat((desc, desc.new_zeros(desc.shape[0], width - desc.shape[1])), 1)
        cloud = cloud if isinstance(cloud, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(cloud)[:, :3], dtype=np.float32))
        self.fragments[int(fragment_id)] = (kp.contiguous(), desc.contiguous(), count,
                                            cloud.to(self.device, torch.float32)[:, :3].contiguous())
        self._bank = self._refine_bank = None
        return self.fragments[int(fragment_id)]

    def add_fragment(self, fragment_id, pc, sn, node, cloud):
        keypoints, sigmas = inference.run_model(self.detector, pc, sn, node)
        kp, count = select_keypoints_device(keypoints, sigmas, self.nms_radius, self.top)
        desc = inference.describe_keypoints(self.descriptor, pc, sn, kp)
        return self._store(fragment_id, kp[0], desc[0], count[0], cloud)

    def add_fragment_keypoints(self, fragment_id, pc, sn, kp, count, cloud):
        """Keypoints from elsewhere (usip_amd.baselines: ISS, Harris3D, SIFT3D, random) instead of the detector's: kp f32 [1,3,M'] with M' <=
        top, count i32 [1] on the device.  Described and cached exactly as add_fragment does."""
        if kp.dim() != 3 or kp.shape[0] != 1 or kp.shape[1] != 3 or kp.shape[2] < 1:
            raise ValueError("add_fragment_keypoints: expected kp [1,3,M'], got %s" % (tuple(kp.shape),))
        kp = kp.to(self.device, torch.float32).contiguous()
        count = torch.clamp(count.to(self.device, torch.int32).reshape(1), max=kp.shape[2])
        desc = inference.describe_keypoints(self.descriptor, pc, sn, kp)
        return self._store(fragment_id, kp[0], desc[0], count[0], cloud)

    def add_fragment_result(self, fragment_id, xyz, desc, cloud):
        xyz = torch.as_tensor(np.asarray(xyz, np.float32) if not isinstance(xyz, torch.Tensor) else xyz).to(self.device, torch.float32)
        desc = torch.as_tensor(np.asarray(desc, np.float32) if not isinstance(desc, torch.Tensor) else desc).to(self.device, torch.float32)
        count = torch.tensor(xyz.shape[0], dtype=torch.int32, device=self.device)
        return self._store(fragment_id, xyz.t(), desc.t(), count, cloud)

    def add_described(self, fragment_ids, kp, desc, count, clouds):
        """A batch described elsewhere (fragment_batch.FragmentDescriber): kp f32 [B,3,M'], desc f32 [B,D,M'], count i32 [B]
        on the device, clouds: every fragment's full cloud.  Cached as add_fragment caches one; nothing is read back."""
        ids = [int(i) for i in fragment_ids]
        if kp.dim() != 3 or desc.dim() != 3 or kp.shape[0] != len(ids) or desc.shape[0] != len(ids) or kp.shape[1] != 3 or \
                desc.shape[2] != kp.shape[2] or count.numel() != len(ids) or len(clouds) != len(ids):
            raise ValueError("add_described: expected kp [B,3,M'], desc [B,D,M'], count [B] and B clouds for %d ids" % len(ids))
        kp, desc = kp.to(self.device, torch.float32), desc.to(self.device, torch.float32)
        count = torch.clamp(count.to(self.device, torch.int32).reshape(-1), max=kp.shape[2])
        return [self._store(i, kp[b], desc[b], count[b], clouds[b]) for b, i in enumerate(ids)]

    def fragment_arrays(self, fragment_id):
        """(xyz [M',3], desc [M',D]) of a cached fragment on the host: what write_descriptors_bin takes."""
        kp, desc, count, _ = self.fragments[int(fragment_id)]
        n = int(count)
        return kp[:, :n].t().cpu().numpy(), desc[:, :n].t().cpu().numpy()

    def ids(self) -> List[int]:
        return sorted(self.fragments)

    def bank(self) -> FragmentBank:
        if self._bank is None:
            self._bank = FragmentBank([self.fragments[i][3] for i in self.ids()], self.device)
        return self._bank

    def refine_bank(self) -> Optional[RefineBank]:
        """The downsampled fragments beside bank(), when refine is on; built once (it reads every fragment's row count)."""
        if self.refine and self._refine_bank is None:
            self._refine_bank = RefineBank([self.fragments[i][3] for i in self.ids()], self.device, self.refine_leaf,
                                           normals=self.refine_metric == "point_to_plane")
        return self._refine_bank

    def all_pairs(self):
        ids = self.ids()
        return [(a, b) for x, a in enumerate(ids) for b in ids[x + 1:]]

    def stacked(self):
        """(kp f32 [F,3,top], desc f32 [F,D,top], count i32 [F]) over the fragments in id order."""
        fr = [self.fragments[i] for i in self.ids()]
        return torch.stack([f[0] for f in fr]), torch.stack([f[1] for f in fr]), torch.stack([f[2] for f in fr])

    def evaluate_device(self, pairs: Optional[Sequence] = None, gt: Optional[Sequence] = None,
                        gt_info: Optional[Sequence] = None) -> Dict[str, torch.Tensor]:
        """Every pair through register_pairs, batch by batch -> per-pair device tensors; nothing synchronises.  With
        optimize the scene's graph is built from them and optimised here too (gt, gt_info: what fill "gt" fills from)."""
        pairs = self.all_pairs() if pairs is None else list(pairs)
        dense = None
        if self.optimize:
            from . import posegraph
            dense = float(self.optimize_args.get("radius", posegraph.INFORMATION_RADIUS))
            plan = posegraph.plan_for(pairs, self.ids(), gt, gt_info, self.optimize_args)   # a chain that cannot close: here
        slot = {i: s for s, i in enumerate(self.ids())}
        bank, fine = self.bank(), self.refine_bank()
        kp, desc, cnt = self.stacked()
        parts = []
        for base in range(0, len(pairs), self.batch_pairs):
            chunk = pairs[base:base + self.batch_pairs]
            f1 = torch.tensor([slot[int(a)] for a, _ in chunk], dtype=torch.int32).to(self.device, non_blocking=True)
            f2 = torch.tensor([slot[int(b)] for _, b in chunk], dtype=torch.int32).to(self.device, non_blocking=True)
            ids = torch.arange(base, base + len(chunk), dtype=torch.int64, device=self.device)
            a, b = f1.long(), f2.long()
            parts.append(register_pairs(kp[a], desc[a], cnt[a].contiguous(), kp[b], desc[b], cnt[b].contiguous(), bank, f1,
                                        f2, ids, self.k, self.inlier_threshold, self.max_trials, self.overlap_radius,
                                        self.seed, self.registrator, fine, self.refine_args, dense, self.refine_metric))
        if not parts:
            return {}
        out = {key: torch.cat([p[key] for p in parts]) for key in parts[0]}
        if self.optimize:
            out.update(posegraph.prune_pairs(plan, out["gate_refined"], out[self._log_key()], out["dense_information"],
                                             self.optimize_args))
        return out

    def _log_key(self):
        return "refined_Rt" if self.log_transform == "refined" else "Rt"

    def evaluate(self, pairs: Optional[Sequence] = None, gt: Optional[Sequence] = None,
                 gt_info: Optional[Sequence] = None) -> Dict:
        dev = self.evaluate_device(pairs, gt, gt_info)
        host = {k: v.cpu().numpy() for k, v in dev.items()}                # the one read
        return summarize(host, self.ids(), gt, gt_info, None, "gate_refined" if self.refine else "gate", self._log_key(),
                         self.optimize_args if self.optimize else None)


def summarize(per_pair: Dict[str, np.ndarray], fragment_ids: Sequence[int], gt=None, gt_info=None,
              num_fragments: Optional[int] = None, gate: str = "gate", transform: str = "Rt",
              optimize_args: Optional[Dict] = None) -> Dict:
    """What evaluate.m prints (when gt and gt_info are given) plus the result log's entries and the per-pair arrays.
    optimize_args (a dict, possibly empty; per_pair must hold dense_information): the result log's pairs as a pose graph,
    its loop closures pruned (posegraph.summarize_loops; run on the host twins here unless per_pair already holds
    loop_kept) -> also loop_recall, loop_precision, loops_in, loops_kept, refined_entries and split."""
    n = int(num_fragments if num_fragments is not None else (gt[0].info[2] if gt else len(fragment_ids)))
    entries = result_entries(per_pair, fragment_ids, n, gate, transform) if per_pair else []
    out = {"pairs": int(len(per_pair[gate])) if per_pair else 0, "written": len(entries), "entries": entries,
           "per_pair": per_pair}
    if gt is not None and gt_info is not None:
        out.update(evaluate_log(entries, gt, gt_info))
    if optimize_args is not None and per_pair:
        from . import posegraph
        out.update(posegraph.summarize_loops(per_pair, fragment_ids, gt, gt_info, gate, transform, optimize_args))
    return out


# ------------------------------------------------------------------------------------------------ a synthetic scene
def synthetic_scene(seed: int = 0, fragments: int = 6, points: int = 20000, dim: int = 128, span: float = 5.0,
                    step: float = 1.0, landmarks: Optional[int] = None, ground_truth: bool = True):
    """A room of planes and boxes cut into overlapping posed fragments, with the ground truth the benchmark's files hold.

    The room is `span + (fragments - 1) step` long; fragment i holds the surface points and the landmarks of the slab
    [i step, i step + span] along the room, expressed in its own frame (a random rigid pose).  Landmark l carries the
    one-hot descriptor l, so overlapping fragments share exact correspondences; with `landmarks` given there are that
    many, each with a random unit descriptor.  -> dict(clouds [f32 [n,3]], xyz, desc (per fragment), poses [4x4, fragment
    -> world], gt (LogEntry, pairs overlapping >= 30 %), gt_info (InfoEntry)); ground_truth False leaves gt, gt_info empty."""
    rng = np.random.default_rng(seed)
    length, width, height = span + (fragments - 1) * step, 4.0, 2.6
    total = int(points * length / span)
    # surfaces: floor, ceiling, two long walls, and boxes standing on the floor
    boxes = [(rng.uniform(0.3, length - 0.9), rng.uniform(0.2, width - 1.0), rng.uniform(0.4, 0.8), rng.uniform(0.4, 0.8),
              rng.uniform(0.4, 1.2)) for _ in range(2 * fragments + 4)]
    areas = [length * width] * 2 + [length * height] * 2 + [2 * (bx * bz + by * bz) + bx * by for _, _, bx, by, bz in boxes]
    share = np.asarray(areas) / np.sum(areas)
    parts = []
    for s, n in enumerate(rng.multinomial(total, share)):
        u, v = rng.uniform(size=n), rng.uniform(size=n)
        if s == 0:
            parts.append(np.stack((u * length, v * width, np.zeros(n)), 1))
        elif s == 1:
            parts.append(np.stack((u * length, v * width, np.full(n, height)), 1))
        elif s == 2:
            parts.append(np.stack((u * length, np.zeros(n), v * height), 1))
        elif s == 3:
            parts.append(np.stack((u * length, np.full(n, width), v * height), 1))
        else:
            x0, y0, bx, by, bz = boxes[s - 4]
            face = rng.integers(0, 5, size=n)
            p = np.stack((x0 + u * bx, y0 + v * by, np.full(n, bz)), 1)                    # top
            side = np.stack((x0 + u * bx, np.where(face == 1, y0, y0 + by), v * bz), 1)
            p = np.where(((face == 1) | (face == 2))[:, None], side, p)
            side = np.stack((np.where(face == 3, x0, x0 + bx), y0 + u * by, v * bz), 1)
            p = np.where(((face == 3) | (face == 4))[:, None], side, p)
            parts.append(p)
    world = np.concatenate(parts)
    world = world[rng.permutation(len(world))]
    marks = world[rng.choice(len(world), dim if landmarks is None else int(landmarks), replace=False)]
    if landmarks is None:
        codes = np.eye(dim, dtype=np.float32)
    else:
        codes = rng.normal(size=(int(landmarks), dim))
        codes = (codes / np.linalg.norm(codes, axis=1, keepdims=True)).astype(np.float32)
    clouds, xyz, desc, poses = [], [], [], []
    for i in range(fragments):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.2, 1.0)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, rng.uniform(-2, 2, size=3)                               # fragment -> world
        poses.append(T)
        inv = np.linalg.inv(T)
        lo, hi = i * step, i * step + span
        pts = world[(world[:, 0] >= lo) & (world[:, 0] <= hi)]
        clouds.append(np.ascontiguousarray((pts @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)))
        seen = np.nonzero((marks[:, 0] >= lo) & (marks[:, 0] <= hi))[0]
        xyz.append(np.ascontiguousarray((marks[seen] @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)))
        desc.append(codes[seen])
    gt, gt_info = [], []
    for i in range(fragments if ground_truth else 0):
        for j in range(i + 1, fragments):
            trans = np.linalg.inv(poses[i]) @ poses[j]                                      # fragment j -> fragment i
            a = clouds[i].astype(np.float64)
            b = clouds[j].astype(np.float64) @ trans[:3, :3].T + trans[:3, 3]
            near = _has_neighbour(a, b, 0.05)
            if near.mean() < 0.3:
                continue
            gt.append(LogEntry((i, j, fragments), trans))
            gt_info.append(InfoEntry((i, j, fragments), information_numpy(a[near])))
    return dict(clouds=clouds, xyz=xyz, desc=desc, poses=poses, gt=gt, gt_info=gt_info)


def _has_neighbour(a, b, cell):
    """For every row of a: does b have a row in the same or an adjacent grid cell of size `cell` (so within cell .. 2 cell
    per axis)?  Host numpy; only the synthetic scene's ground truth is built from it."""
    origin = np.floor(np.minimum(a.min(0), b.min(0)) / cell).astype(np.int64) - 1
    ka, kb = np.floor(a / cell).astype(np.int64) - origin, np.floor(b / cell).astype(np.int64) - origin
    m = int(max(ka.max(), kb.max())) + 3
    occupied = np.unique((kb[:, 0] * m + kb[:, 1]) * m + kb[:, 2])
    out = np.zeros(len(a), bool)
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                out |= np.isin(((ka[:, 0] + x) * m + ka[:, 1] + y) * m + ka[:, 2] + z, occupied)
    return out


def information_numpy(points):
    """register2Fragments.m:78-87 over `points` [n,3]: the sum of A'A, float64 host numpy."""
    s = np.asarray(points, np.float64).reshape(-1, 3)
    A = np.zeros((len(s), 3, 6))
    A[:, 0, 0] = A[:, 1, 1] = A[:, 2, 2] = 1.0
    A[:, 0, 4], A[:, 0, 5] = 2 * s[:, 2], -2 * s[:, 1]
    A[:, 1, 3], A[:, 1, 5] = -2 * s[:, 2], 2 * s[:, 0]
    A[:, 2, 3], A[:, 2, 4] = 2 * s[:, 1], -2 * s[:, 0]
    return np.einsum("nki,nkj->ij", A, A)
