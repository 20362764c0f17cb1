"""Evaluation on the device: the two numbers a trained USIP model is judged by.

  match_descriptors      pdist2(pos_desc, anc_desc, 'euclidean', 'smallest', 1) of evaluate_kitti.m on ragged batches
  ransac_registration    external/ransacfitRt.m + ransac.m + estimateRt.m + estimateRigidTransform.m, and
                         Utils.compareTransform when a ground truth is given
  repeatability          the last lines of eval_repeatability/eval_rep.m
  compare_transform      Utils.compareTransform
  RegistrationEvaluator  detector -> NMS / top-k -> descriptor per frame, cached on the device; evaluate(pairs) prints
                         what evaluate_kitti.m and eval_rep.m print
  *_cpu                  the same on numpy arrays over the library's host twins (csrc/registration_cpu.cpp)

RANSAC here is the reference's algorithm with its OWN draws: ransac.m calls rng(0) and MATLAB's randsample, a stream that
cannot be reproduced, so trial t of pair g draws its triplet from Philox4x64-10 keyed by (seed, g, t)
(csrc/registration_math.h).  Because a trial's score does not depend on the trials before it, all max_trials + 1 scores
are computed in parallel and ransac.m's sequential stopping rule is replayed over them: the chosen trial and the trial
count are those of the serial algorithm on the same draws.
"""
import ctypes
from collections import namedtuple
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, inference, ops

RegistrationResult = namedtuple("RegistrationResult", "Rt inliers inlier_mask trialcount valid delta_t delta_deg chosen counts")


def match_descriptors(anc_desc, pos_desc, anc_count, pos_count) -> torch.Tensor:
    """anc_desc f32 [P,C,Ma], pos_desc f32 [P,C,Mp], counts i32 [P] -> idx i32 [P,Ma]: for every anchor descriptor the
    FIRST index of the nearest positive descriptor (rows beyond anc_count: 0)."""
    return ops.nearest_nd_counted(anc_desc, pos_desc, anc_count, pos_count)[1]


def ransac_registration(x1, x2, count, threshold: float = 1.0, max_trials: int = 10000, seed: int = 0, pair_ids=None,
                        triplets=None, gt=None) -> RegistrationResult:
    """x1 = R x2 + t from matched coordinates x1, x2 f32 [P,3,Nmax] with count i32 [P] (Nmax <= 1024).  pair_ids i64 [P]:
    the global ids the draws are keyed by (default 0..P-1); triplets i32 [P, max_trials + 1, 3]: explicit draws instead;
    gt f64 [P,3,4]: also delta_t, delta_deg (an invalid pair gets the reference's (3, 6)).  Device tensors, no host
    synchronisation."""
    T = int(max_trials) + 1 if triplets is None else int(triplets.shape[1])
    counts, _, _ = ops.ransac_trials(x1, x2, count, T, threshold, seed, pair_ids, triplets)
    o = ops.ransac_select(x1, x2, count, counts, min(int(max_trials), T - 1), threshold, seed, pair_ids, triplets, gt)
    return RegistrationResult(o["Rt"], o["inliers"], o["inlier_mask"], o["trialcount"], o["valid"], o["delta_t"],
                              o["delta_deg"], o["chosen"], counts)


def repeatability(anc_kp, anc_count, pos_kp, pos_count, gt, radius: float = 0.5):
    """-> (ratio f64 [P], hits i32 [P], min_dist f64 [P,Ma]): the share of anchor keypoints with a positive keypoint,
    moved by gt, closer than radius."""
    md, hits, ratio = ops.repeatability(anc_kp, anc_count, pos_kp, pos_count, gt, radius)
    return ratio, hits, md


def compare_transform(gt, Rt):
    """gt, Rt f64 [P,3,4] -> (delta_t, delta_deg) f64 [P]."""
    return ops.compare_transform(gt, Rt)


# ------------------------------------------------------------------------------------------------ host twins (numpy)
def _np(a, dtype, name, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("%s must have shape %s (got %s)" % (name, tuple(shape), a.shape))
    return a


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _pairs_np(x1, x2, count, limit):
    x1, x2 = _np(x1, np.float32, "x1"), _np(x2, np.float32, "x2")
    if x1.ndim != 3 or x1.shape[1] != 3 or x2.shape != x1.shape:
        raise ValueError("expected x1, x2 [P,3,Nmax]")
    if not 1 <= x1.shape[2] <= limit:                              # the device entries' rule and error (ops._need_pairs)
        raise RuntimeError("registration: Nmax must be in 1..%d (got %d)" % (limit, x1.shape[2]))
    return x1, x2, _np(count, np.int32, "count", (x1.shape[0],))


def ransac_trials_cpu(x1, x2, count, T: int, threshold: float = 1.0, seed: int = 0, pair_ids=None, triplets=None,
                      num_threads: int = 1, _nmax: int = ops.RANSAC_NMAX):
    """-> (counts i32 [P,T], hypotheses f64 [P,T,3,4], triplets i32 [P,T,3]) on the host."""
    x1, x2, count = _pairs_np(x1, x2, count, _nmax)
    P, _, Nmax = x1.shape
    T = int(T)
    ids = _np(pair_ids, np.int64, "pair_ids", (P,)) if pair_ids is not None else None
    tri = _np(triplets, np.int32, "triplets", (P, T, 3)) if triplets is not None else None
    counts = np.zeros((P, T), np.int32)
    hyp = np.zeros((P, T, 3, 4), np.float64)
    drawn = np.zeros((P, T, 3), np.int32)
    _lib.check(_lib.lib().usip_ransac_trials_f32_cpu(_p(x1), _p(x2), _p(count), P, Nmax, T, float(threshold),
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _p(ids), _p(tri), _p(counts), _p(hyp),
                                                     _p(drawn), int(num_threads)), "usip_ransac_trials_f32_cpu")
    return counts, hyp, drawn


def ransac_select_cpu(x1, x2, count, counts, max_trials: int, threshold: float = 1.0, seed: int = 0, pair_ids=None,
                      triplets=None, gt=None, _nmax: int = ops.RANSAC_NMAX) -> Dict[str, np.ndarray]:
    x1, x2, count = _pairs_np(x1, x2, count, _nmax)
    P, _, Nmax = x1.shape
    counts = _np(counts, np.int32, "counts")
    T = counts.shape[1]
    ids = _np(pair_ids, np.int64, "pair_ids", (P,)) if pair_ids is not None else None
    tri = _np(triplets, np.int32, "triplets", (P, T, 3)) if triplets is not None else None
    g = _np(gt, np.float64, "gt", (P, 3, 4)) if gt is not None else None
    o = {"Rt": np.zeros((P, 3, 4)), "inlier_mask": np.zeros((P, Nmax), np.uint8), "inliers": np.zeros(P, np.int32),
         "trialcount": np.zeros(P, np.int32), "valid": np.zeros(P, np.uint8), "chosen": np.zeros(P, np.int32),
         "delta_t": np.zeros(P) if g is not None else None, "delta_deg": np.zeros(P) if g is not None else None}
    _lib.check(_lib.lib().usip_ransac_select_f32_cpu(
        _p(x1), _p(x2), _p(count), P, Nmax, T, int(max_trials), float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(ids),
        _p(tri), _p(counts), _p(g), _p(o["Rt"]), _p(o["inlier_mask"]), _p(o["inliers"]), _p(o["trialcount"]),
        _p(o["valid"]), _p(o["chosen"]), _p(o["delta_t"]), _p(o["delta_deg"])), "usip_ransac_select_f32_cpu")
    return o


def ransac_registration_cpu(x1, x2, count, threshold: float = 1.0, max_trials: int = 10000, seed: int = 0, pair_ids=None,
                            triplets=None, gt=None, num_threads: int = 1) -> RegistrationResult:
    T = int(max_trials) + 1 if triplets is None else int(np.shape(triplets)[1])
    counts, _, _ = ransac_trials_cpu(x1, x2, count, T, threshold, seed, pair_ids, triplets, num_threads)
    o = ransac_select_cpu(x1, x2, count, counts, min(int(max_trials), T - 1), threshold, seed, pair_ids, triplets, gt)
    return RegistrationResult(o["Rt"], o["inliers"], o["inlier_mask"], o["trialcount"], o["valid"], o["delta_t"],
                              o["delta_deg"], o["chosen"], counts)


def compare_transform_cpu(gt, Rt):
    gt, Rt = _np(gt, np.float64, "gt"), _np(Rt, np.float64, "Rt")
    if gt.ndim != 3 or gt.shape[1:] != (3, 4) or Rt.shape != gt.shape:
        raise ValueError("expected gt, Rt [P,3,4]")
    P = gt.shape[0]
    dt, dd = np.zeros(P), np.zeros(P)
    _lib.check(_lib.lib().usip_compare_transform_f64_cpu(_p(gt), _p(Rt), P, _p(dt), _p(dd)),
               "usip_compare_transform_f64_cpu")
    return dt, dd


def repeatability_cpu(anc_kp, anc_count, pos_kp, pos_count, gt, radius: float = 0.5):
    anc, pos = _np(anc_kp, np.float32, "anc_kp"), _np(pos_kp, np.float32, "pos_kp")
    P, _, Ma = anc.shape
    Mp = pos.shape[2]
    ac, pc = _np(anc_count, np.int32, "anc_count", (P,)), _np(pos_count, np.int32, "pos_count", (P,))
    g = _np(gt, np.float64, "gt", (P, 3, 4))
    md, hits, ratio = np.zeros((P, Ma)), np.zeros(P, np.int32), np.zeros(P)
    _lib.check(_lib.lib().usip_repeatability_f32_cpu(_p(anc), _p(ac), _p(pos), _p(pc), _p(g), float(radius), P, Ma, Mp,
                                                     _p(md), _p(hits), _p(ratio)), "usip_repeatability_f32_cpu")
    return ratio, hits, md


def match_descriptors_cpu(anc_desc, pos_desc, anc_count, pos_count):
    a, b = _np(anc_desc, np.float32, "anc_desc"), _np(pos_desc, np.float32, "pos_desc")
    B, C, Ma = a.shape
    Nb = b.shape[2]
    ac, bc = _np(anc_count, np.int32, "anc_count", (B,)), _np(pos_count, np.int32, "pos_count", (B,))
    d, arg = np.zeros((B, Ma), np.float32), np.zeros((B, Ma), np.int32)
    _lib.check(_lib.lib().usip_nearest_nd_counted_f32_cpu(_p(a), _p(b), _p(ac), _p(bc), _p(d), _p(arg), B, C, Ma, Nb),
               "usip_nearest_nd_counted_f32_cpu")
    return arg


# ------------------------------------------------------------------------------------------------ the evaluator
def select_keypoints_device(keypoints: torch.Tensor, sigmas: torch.Tensor, nms_radius: float, top: int):
    """inference.select_keypoints' rule kept on the device: -> (kp f32 [B,3,top] padded with the frame's first pick,
    count i32 [B])."""
    B, _, M = keypoints.shape
    top = min(int(top), M)
    if nms_radius < 0.01:
        order = torch.argsort(sigmas, dim=1, stable=True)
        count = torch.full((B,), top, dtype=torch.int32, device=keypoints.device)
    else:
        order, count = ops.nms(keypoints.contiguous(), sigmas.contiguous(), nms_radius)
        order, count = order.long(), torch.clamp(count, max=top)
    order = order[:, :top]
    slot = torch.arange(top, device=keypoints.device).unsqueeze(0)
    order = torch.where(slot < count.unsqueeze(1), order, order[:, :1])
    kp = torch.gather(keypoints, 2, order.unsqueeze(1).expand(-1, 3, -1)).contiguous()
    return kp, count.to(torch.int32)


class RegistrationEvaluator:
    """Scores a detector + descriptor pair the way the reference's MATLAB does, without leaving the device.

    add_frame(id, pc, sn, node) runs detector -> NMS / top-k -> descriptor on one frame ([1,3,N], [1,Cs,N], [1,3,M]
    device tensors) and caches its keypoints f32 [3,top], descriptors f32 [D,top] and count; add_frame_keypoints(id, pc,
    sn, kp, count) takes a baseline detector's keypoints instead (the detector may then be None); add_frame_descriptors(id,
    kp, desc, count) takes descriptors computed elsewhere too (baselines.FpfhDescriptor: both may be None).  evaluate(pairs) with
    pairs = [(anc_id, pos_id, T_gt 3x4 mapping the positive frame into the anchor's)] matches descriptors, runs RANSAC
    and repeatability in batches and returns evaluate_kitti.m's and eval_rep.m's printed quantities; the poses are in
    the frame the keypoints are in.  One host read at the end."""

    def __init__(self, detector, descriptor, opt, device, nms_radius: float = 2.0, top: int = 512,
                 inlier_threshold: float = 1.0, max_trials: int = 10000, repeat_radius: float = 0.5, seed: int = 0,
                 batch_pairs: int = 64):
        self.detector, self.descriptor, self.opt = detector, descriptor, opt
        self.device = torch.device(device)
        self.nms_radius, self.top = float(nms_radius), int(top)
        self.inlier_threshold, self.max_trials = float(inlier_threshold), int(max_trials)
        self.repeat_radius, self.seed, self.batch_pairs = float(repeat_radius), int(seed), int(batch_pairs)
        self.frames = {}

    def add_frame(self, frame_id, pc, sn, node):
        keypoints, sigmas = inference.run_model(self.detector, pc, sn, node)
        kp, count = select_keypoints_device(keypoints, sigmas, self.nms_radius, self.top)
        desc = inference.describe_keypoints(self.descriptor, pc, sn, kp)
        return self._cache(frame_id, kp, desc, count)

    def _cache(self, frame_id, kp, desc, count):
        """kp [1,3,M'], desc [1,D,M'], count [1] with M' <= top -> the cached (kp [3,top], desc [D,top], count)"""
        width = self.top
        if kp.shape[2] < width:                                   # fewer nodes than top: pad to one width for batching
            kp = torch.cat((kp, kp[:, :, :1].expand(-1, -1, width - kp.shape[2])), 2)
            desc = torch.cat((desc, desc[:, :, :1].expand(-1, -1, width - desc.shape[2])), 2)
        self.frames[frame_id] = (kp[0].contiguous(), desc[0].contiguous(), count[0])
        return self.frames[frame_id]

    def add_frame_keypoints(self, frame_id, pc, sn, kp, count):
        """Keypoints from elsewhere (usip_amd.baselines: ISS, Harris3D, SIFT3D, random) instead of the detector's: kp f32 [1,3,M'] with M' <=
        top, count i32 [1] on the device.  Described and cached exactly as add_frame does."""
        if kp.dim() != 3 or kp.shape[0] != 1 or kp.shape[1] != 3 or not 1 <= kp.shape[2] <= self.top:
            raise ValueError("add_frame_keypoints: expected kp [1,3,M'] with 1 <= M' <= top = %d, got %s"
                             % (self.top, tuple(kp.shape)))
        kp = kp.to(self.device, torch.float32).contiguous()
        count = torch.clamp(count.to(self.device, torch.int32).reshape(1), max=kp.shape[2])
        desc = inference.describe_keypoints(self.descriptor, pc, sn, kp)
        return self._cache(frame_id, kp, desc, count)

    def add_frame_descriptors(self, frame_id, kp, desc, count):
        """Keypoints AND descriptors from elsewhere (usip_amd.baselines.FpfhDescriptor on a baseline detector's keypoints): kp
        f32 [1,3,M'], desc f32 [1,D,M'] with M' <= top, count i32 [1] on the device.  Padded and cached exactly as
        add_frame_keypoints does; the evaluator's detector and descriptor may both be None."""
        if kp.dim() != 3 or kp.shape[0] != 1 or kp.shape[1] != 3 or not 1 <= kp.shape[2] <= self.top:
            raise ValueError("add_frame_descriptors: expected kp [1,3,M'] with 1 <= M' <= top = %d, got %s"
                             % (self.top, tuple(kp.shape)))
        if desc.dim() != 3 or desc.shape[0] != 1 or desc.shape[1] < 1 or desc.shape[2] != kp.shape[2]:
            raise ValueError("add_frame_descriptors: expected desc [1,D,%d], got %s" % (kp.shape[2], tuple(desc.shape)))
        kp = kp.to(self.device, torch.float32).contiguous()
        desc = desc.to(self.device, torch.float32).contiguous()
        count = torch.clamp(count.to(self.device, torch.int32).reshape(1), max=kp.shape[2])
        return self._cache(frame_id, kp, desc, count)

    def frame_arrays(self, frame_id) -> Tuple[np.ndarray, np.ndarray]:
        """(xyz [M',3], desc [M',D]) of a cached frame on the host: what write_descriptors_bin takes."""
        kp, desc, count = self.frames[frame_id]
        n = int(count)
        return kp[:, :n].t().cpu().numpy(), desc[:, :n].t().cpu().numpy()

    def _batch(self, pairs, base: int):
        dev = self.device
        A = [self.frames[p[0]] for p in pairs]
        Q = [self.frames[p[1]] for p in pairs]
        anc_kp, pos_kp = torch.stack([f[0] for f in A]), torch.stack([f[0] for f in Q])
        anc_desc, pos_desc = torch.stack([f[1] for f in A]), torch.stack([f[1] for f in Q])
        anc_n, pos_n = torch.stack([f[2] for f in A]), torch.stack([f[2] for f in Q])
        gt = torch.from_numpy(np.stack([np.asarray(p[2], dtype=np.float64).reshape(3, 4) for p in pairs])).to(dev)
        idx = match_descriptors(anc_desc, pos_desc, anc_n, pos_n)
        x2 = torch.gather(pos_kp, 2, idx.long().unsqueeze(1).expand(-1, 3, -1)).contiguous()
        count = torch.where(pos_n > 0, anc_n, torch.zeros_like(anc_n))      # no positive keypoints: nothing matched
        ids = torch.arange(base, base + len(pairs), dtype=torch.int64, device=dev)
        reg = ransac_registration(anc_kp, x2, count, self.inlier_threshold, self.max_trials, self.seed, ids, None, gt)
        ratio, hits, _ = repeatability(anc_kp, anc_n, pos_kp, pos_n, gt, self.repeat_radius)
        return dict(delta_t=reg.delta_t, delta_deg=reg.delta_deg, inliers=reg.inliers, trialcount=reg.trialcount,
                    valid=reg.valid, matches=count, repeatability=ratio, keypoint_num=anc_n, Rt=reg.Rt, match_idx=idx)

    def evaluate(self, pairs: Sequence) -> Dict:
        pairs = list(pairs)
        parts = [self._batch(pairs[i:i + self.batch_pairs], i) for i in range(0, len(pairs), self.batch_pairs)]
        host = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in parts[0]} if parts else {}   # the one read
        return summarize(host) if parts else summarize(None)


def summarize(per_pair: Optional[Dict[str, np.ndarray]]) -> Dict:
    """evaluate_kitti.m's and eval_rep.m's printed quantities from per-pair arrays (MATLAB std: n - 1; a mean over no
    pair is NaN as in MATLAB)."""
    if per_pair is None:
        per_pair = {k: np.zeros(0) for k in ("delta_t", "delta_deg", "inliers", "trialcount", "matches", "repeatability",
                                             "keypoint_num")}
    dt, dd = per_pair["delta_t"], per_pair["delta_deg"]
    wrong = (dt > 2) | (dd > 5)
    good = ~wrong

    def mean(a):
        return float(np.mean(a)) if a.size else float("nan")

    def std(a):
        return float(np.std(a, ddof=1)) if a.size > 1 else (0.0 if a.size == 1 else float("nan"))

    ratio = per_pair["inliers"][good] / np.maximum(per_pair["matches"][good], 1)
    rep = per_pair["repeatability"]
    return {"pairs": int(dt.size), "wrong": int(wrong.sum()),
            "inlier_ratio_mean": mean(ratio), "trial_count_mean": mean(per_pair["trialcount"][good].astype(np.float64)),
            "rte_mean": mean(dt[good]), "rte_std": std(dt[good]), "rre_mean": mean(dd[good]), "rre_std": std(dd[good]),
            "repeatability_mean": mean(rep), "repeatability_min": float(rep.min()) if rep.size else float("nan"),
            "repeatability_max": float(rep.max()) if rep.size else float("nan"),
            "keypoint_num_mean": mean(per_pair["keypoint_num"].astype(np.float64)), "per_pair": per_pair}
