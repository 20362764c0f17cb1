"""A fragment scene's ground truth on the device: gt.log and gt.info, the files every indoor number is scored
against (evaluation/matlab/eval_indoor/3dmatch/getGtInfoLog.m), and the indoor repeatability pair list that
evaluation/matlab/eval_repeatability/build_3dmatch_dataset.m reads out of the same gt.log.

  reach                        for every row of fragment j moved by relExt: does fragment i have a row within 0.03 m (class 1)
                               or 0.006 m (class 2)?  One bounded walk (csrc/ground_truth.hip) answers both, with the counts,
                               alignedRatio and a selection key per class-2 row
  correspondence_information   covMat: the class-2 rows, thinned to the `cap` smallest (key, row) by a stable device sort, the
                               sum of G'G, G = [I3 | -[q]x], over them
  scene_ground_truth           all pairs i < j of a scene in batches, the host read once -> gt, gt_info, per_pair
  *_cpu                        the same on numpy arrays over the library's host twins (csrc/ground_truth_cpu.cpp)
  read_fragment_pose / write_scene_ground_truth    cloud_bin_<i>.info.txt in, <scene>-evaluation/gt.log and gt.info out
  repeatability_pairs / scene_repeatability        build_3dmatch_dataset.m's list; eval_rep.m per listed pair over f-6's kernel

Deviations from getGtInfoLog.m: the thinning is a keyed selection, not pcdownsample 'random'; distances are
float64 on the float32 rows; both comparisons are the strict sqrt(d2) < radius.
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, evaluation, fragments, ops
from .evaluation import _np, _p
from .fragments import FragmentBank, HostBank, InfoEntry, LogEntry, RefineBank

LEAF, FAR, NEAR, CAP, MIN_RATIO = 0.01, 0.03, 0.006, 5000, 0.3             # getGtInfoLog.m
WORKSPACE_BYTES = 1 << 30                                                   # what a batch's per-row buffers may take
SLOT_BYTES = 64     # per pair and row of the longest fragment: moved x 8, its argsort 8, perm2 4, cls 1, key 8, the key sort 24
VOXEL_POINTS_MAX, VOXEL_CELLS_MAX = 1 << 20, 1 << 20                        # scan_voxel_keys: rows per cloud, cells per axis
_SIGN = -(1 << 63)


# ------------------------------------------------------------------------------------------------ device
def reach(bank: FragmentBank, frag1, frag2, Rt, far: float = FAR, near: float = NEAR, seed: int = 0, pair_ids=None, mask=None):
    """frag1, frag2 i32 [P] (fragments of the bank), Rt f64 [P,3,4] moving fragment 2 into fragment 1's frame -> dict(cls u8
    [P,lmax] in fragment 2's local row order, hits i32 [P,2], ratio f64 [P,2], key i64 [P,lmax]) as ops.gt_reach states them.
    Fragment 2's rows are sorted along their moved x here, on the device.  No host synchronisation."""
    Rt = Rt.contiguous()
    m = None if mask is None else mask.to(torch.uint8).contiguous()
    return ops.gt_reach(bank.rows, bank.offsets, bank.perm, frag1, frag2, Rt, fragments.moved_x_order(bank, frag2, Rt), far,
                        near, seed, pair_ids, m)


def select_rows(key, cap: int = CAP):
    """key i64 [P,lmax] (u64 bit patterns) -> order i32 [P,min(cap, lmax)]: every pair's rows ascending along (key, row), the
    first `cap` of them -- a stable sort of the keys as unsigned numbers (the sign bit flipped), on the device."""
    return torch.sort(key ^ _SIGN, dim=1, stable=True)[1][:, :int(cap)].to(torch.int32).contiguous()


def correspondence_information(bank: FragmentBank, frag1, frag2, Rt, key, hits, cap: int = CAP, want_order: bool = False):
    """key, hits of reach() on the same bank, pairs and Rt -> info f64 [P,6,6]: getGtInfoLog.m's covMat over the class-2 rows,
    the `cap` smallest (key, row) when there are more.  want_order: -> (info, order i32 [P,min(cap, lmax)]).  No host
    synchronisation."""
    order = select_rows(key, cap)
    info = ops.gt_information(bank.rows, bank.offsets, frag2, Rt.contiguous(), order, hits[:, 1].contiguous(), bank.lmax)
    return (info, order) if want_order else info


def batch_size(P: int, lmax: int, batch_pairs: Optional[int] = None, workspace_bytes: int = WORKSPACE_BYTES) -> int:
    """Pairs per batch: batch_pairs, or as many as keep SLOT_BYTES lmax per pair within workspace_bytes (at least one)."""
    if batch_pairs is None:
        batch_pairs = int(workspace_bytes) // (SLOT_BYTES * max(int(lmax), 1))
    return max(1, min(int(batch_pairs), 65535, max(int(P), 1)))


def pairs_ground_truth(bank: FragmentBank, frag1, frag2, Rt, far: float = FAR, near: float = NEAR, cap: int = CAP, seed: int = 0,
                       pair_ids=None, batch_pairs: Optional[int] = None, workspace_bytes: int = WORKSPACE_BYTES):
    """reach and correspondence_information over device tensors frag1, frag2 i32 [P], Rt f64 [P,3,4] in batches -> dict(ratio
    f64 [P,2], hits i32 [P,2], info f64 [P,6,6]) on the device.  pair_ids i64 [P] (None: 0 .. P-1) key the selection, so the
    batch split never changes a result.  Nothing synchronises."""
    P = int(frag2.shape[0])
    ids = torch.arange(P, dtype=torch.int64, device=frag2.device) if pair_ids is None else pair_ids
    step = batch_size(P, bank.lmax, batch_pairs, workspace_bytes)
    ratio, hits, info = [], [], []
    for base in range(0, P, step):
        sl = slice(base, base + step)
        o = reach(bank, frag1[sl], frag2[sl], Rt[sl], far, near, seed, ids[sl])
        info.append(correspondence_information(bank, frag1[sl], frag2[sl], Rt[sl], o["key"], o["hits"], cap))
        ratio.append(o["ratio"])
        hits.append(o["hits"])
    if not P:
        dev = frag2.device
        return {"ratio": torch.zeros((0, 2), dtype=torch.float64, device=dev),
                "hits": torch.zeros((0, 2), dtype=torch.int32, device=dev),
                "info": torch.zeros((0, 6, 6), dtype=torch.float64, device=dev)}
    return {"ratio": torch.cat(ratio), "hits": torch.cat(hits), "info": torch.cat(info)}


# ------------------------------------------------------------------------------------------------ the scene
def scene_pairs(poses) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """poses [F,4,4] (fragment -> world) -> (frag1 i32 [P], frag2 i32 [P], trans f64 [P,4,4]) over all i < j in (i, j) order:
    trans = inv(T_i) T_j, float64 on the host, getGtInfoLog.m's relExt."""
    T = np.asarray(poses, np.float64)
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError("scene_pairs: poses must be [F,4,4] (got %s)" % (T.shape,))
    F = T.shape[0]
    f1 = np.array([i for i in range(F) for _ in range(i + 1, F)], np.int32)
    f2 = np.array([j for i in range(F) for j in range(i + 1, F)], np.int32)
    inv = np.linalg.inv(T) if F else T
    trans = np.stack([inv[i] @ T[j] for i, j in zip(f1, f2)]) if len(f1) else np.zeros((0, 4, 4))
    return f1, f2, trans


def check_voxel_range(clouds: Sequence, leaf: float):
    """scan_voxel_keys holds 2^20 rows per cloud and 2^20 cells per axis: refuse a fragment that does not fit, by name."""
    for f, c in enumerate(clouds):
        a = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        if a.shape[0] > VOXEL_POINTS_MAX:
            raise ValueError("scene_ground_truth: fragment %d has %d rows, scan_voxel_keys holds at most %d per cloud"
                             % (f, a.shape[0], VOXEL_POINTS_MAX))
        if a.shape[0] and not np.all(np.isfinite(a[:, :3])):
            raise ValueError("scene_ground_truth: fragment %d has a coordinate that is not finite" % f)
        if a.shape[0]:
            extent = (a[:, :3].astype(np.float64).max(0) - a[:, :3].astype(np.float64).min(0)).max()
            if np.floor(extent / float(leaf)) + 1 > VOXEL_CELLS_MAX:
                raise ValueError("scene_ground_truth: fragment %d spans %.3f m, more than the %d cells per axis of "
                                 "scan_voxel_keys at leaf %g" % (f, extent, VOXEL_CELLS_MAX, leaf))


def _entries(f1, f2, trans, ratio, info, F: int, min_ratio: float):
    gt, gt_info = [], []
    for p in np.nonzero(ratio[:, 0] >= float(min_ratio))[0]:
        head = (int(f1[p]), int(f2[p]), int(F))
        gt.append(LogEntry(head, trans[p].copy()))
        gt_info.append(InfoEntry(head, info[p].copy()))
    return gt, gt_info


def scene_ground_truth(clouds: Sequence, poses, device, leaf: Optional[float] = LEAF, far: float = FAR, near: float = NEAR,
                       cap: int = CAP, min_ratio: float = MIN_RATIO, seed: int = 0, batch_pairs: Optional[int] = None,
                       workspace_bytes: int = WORKSPACE_BYTES):
    """getGtInfoLog.m for one scene on the device.  clouds: the fragments' rows [n,>=3]; poses [F,4,4] fragment -> world.  The
    clouds are grid-averaged at `leaf` (RefineBank; None: taken as they are).  All pairs i < j go through
    pairs_ground_truth in batches; the host is read once, after the last batch.  -> (gt [LogEntry], gt_info [InfoEntry], the
    pairs with ratio[:, 0] >= min_ratio in (i, j) order; per_pair: dict(frag1, frag2, trans, ratio, hits, info, kept) over all
    pairs, numpy)."""
    f1, f2, trans = scene_pairs(poses)
    if len(clouds) != np.shape(poses)[0]:
        raise ValueError("scene_ground_truth: %d clouds but %d poses" % (len(clouds), np.shape(poses)[0]))
    if leaf is None:
        bank = FragmentBank(clouds, device)
    else:
        check_voxel_range(clouds, leaf)
        bank = RefineBank(clouds, device, leaf)
    dev = bank.device
    d1, d2 = torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)
    Rt = torch.from_numpy(np.ascontiguousarray(trans[:, :3, :])).to(dev)
    o = pairs_ground_truth(bank, d1, d2, Rt, far, near, cap, seed, None, batch_pairs, workspace_bytes)
    P = len(f1)
    flat = torch.cat((o["ratio"], o["hits"].to(torch.float64), o["info"].reshape(P, 36)), 1).cpu().numpy()  # the one read
    ratio, hits, info = flat[:, :2], flat[:, 2:4].astype(np.int32), flat[:, 4:].reshape(P, 6, 6)
    gt, gt_info = _entries(f1, f2, trans, ratio, info, len(clouds), min_ratio)
    return gt, gt_info, dict(frag1=f1, frag2=f2, trans=trans, ratio=ratio.copy(), hits=hits, info=info.copy(),
                             kept=ratio[:, 0] >= float(min_ratio))


# ------------------------------------------------------------------------------------------------ host twins (numpy)
def reach_cpu(bank: HostBank, frag1, frag2, Rt, far: float = FAR, near: float = NEAR, seed: int = 0, pair_ids=None, mask=None,
              prune: bool = True, num_threads: int = 1) -> Dict[str, np.ndarray]:
    """reach on numpy arrays over the host twin; key is uint64 here.  prune False tests all rows of fragment 1."""
    args, alive = fragments._host_bank_args(bank)
    perm1 = _np(bank.perm, np.int32, "perm", (args[-1],))
    f2 = _np(frag2, np.int32, "frag2")
    P, L = f2.shape[0], int(bank.lmax)
    f1, G = _np(frag1, np.int32, "frag1", (P,)), _np(Rt, np.float64, "Rt", (P, 3, 4))
    ids = None if pair_ids is None else _np(pair_ids, np.int64, "pair_ids", (P,))
    m = None if mask is None else _np(np.asarray(mask).astype(np.uint8), np.uint8, "mask", (P,))
    o = {"cls": np.zeros((P, L), np.uint8), "hits": np.zeros((P, 2), np.int32), "ratio": np.zeros((P, 2)),
         "key": np.zeros((P, L), np.uint64)}
    _lib.check(_lib.lib().usip_gt_reach_f32_cpu(*args, _p(perm1), _p(f1), _p(f2), _p(G), _p(m), P, L, float(far), float(near),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, _p(ids), 1 if prune else 0, _p(o["cls"]),
                                                _p(o["hits"]), _p(o["ratio"]), _p(o["key"]), int(num_threads)),
               "usip_gt_reach_f32_cpu")
    return o


def select_rows_cpu(key, cap: int = CAP):
    return np.ascontiguousarray(np.argsort(np.asarray(key, np.uint64), axis=1, kind="stable")[:, :int(cap)].astype(np.int32))


def correspondence_information_cpu(bank: HostBank, frag1, frag2, Rt, key, hits, cap: int = CAP, want_order: bool = False,
                                   num_threads: int = 1):
    args, alive = fragments._host_bank_args(bank)
    f2 = _np(frag2, np.int32, "frag2")
    P = f2.shape[0]
    G = _np(Rt, np.float64, "Rt", (P, 3, 4))
    order = select_rows_cpu(key, cap)
    count = _np(np.asarray(hits)[:, 1], np.int32, "hits", (P,))
    info = np.zeros((P, 6, 6))
    _lib.check(_lib.lib().usip_gt_information_f32_cpu(*args, _p(f2), _p(G), _p(order), _p(count), P, int(bank.lmax),
                                                      order.shape[1], _p(info), int(num_threads)),
               "usip_gt_information_f32_cpu")
    return (info, order) if want_order else info


def pairs_ground_truth_cpu(bank: HostBank, frag1, frag2, Rt, far: float = FAR, near: float = NEAR, cap: int = CAP, seed: int = 0,
                           pair_ids=None, batch_pairs: Optional[int] = None, workspace_bytes: int = WORKSPACE_BYTES,
                           num_threads: int = 1, prune: bool = True) -> Dict[str, np.ndarray]:
    f1, f2, G = np.asarray(frag1, np.int32), np.asarray(frag2, np.int32), np.asarray(Rt, np.float64)
    P = len(f2)
    ids = np.arange(P, dtype=np.int64) if pair_ids is None else np.asarray(pair_ids, np.int64)
    step = batch_size(P, bank.lmax, batch_pairs, workspace_bytes)
    out = {"ratio": np.zeros((P, 2)), "hits": np.zeros((P, 2), np.int32), "info": np.zeros((P, 6, 6))}
    for base in range(0, P, step):
        sl = slice(base, base + step)
        o = reach_cpu(bank, f1[sl], f2[sl], G[sl], far, near, seed, ids[sl], None, prune, num_threads)
        out["info"][sl] = correspondence_information_cpu(bank, f1[sl], f2[sl], G[sl], o["key"], o["hits"], cap,
                                                         num_threads=num_threads)
        out["ratio"][sl], out["hits"][sl] = o["ratio"], o["hits"]
    return out


def scene_ground_truth_cpu(clouds: Sequence, poses, leaf: Optional[float] = LEAF, far: float = FAR, near: float = NEAR,
                           cap: int = CAP, min_ratio: float = MIN_RATIO, seed: int = 0, batch_pairs: Optional[int] = None,
                           workspace_bytes: int = WORKSPACE_BYTES, num_threads: int = 1, bank: Optional[HostBank] = None):
    """scene_ground_truth over the host twins; bank: a HostBank to use instead of building one from the clouds."""
    f1, f2, trans = scene_pairs(poses)
    if len(clouds) != np.shape(poses)[0]:
        raise ValueError("scene_ground_truth_cpu: %d clouds but %d poses" % (len(clouds), np.shape(poses)[0]))
    if bank is None:
        if leaf is None:
            bank = fragments.host_bank(clouds)
        else:
            check_voxel_range(clouds, leaf)
            bank = fragments.refine_bank_cpu(clouds, leaf)
    o = pairs_ground_truth_cpu(bank, f1, f2, trans[:, :3, :], far, near, cap, seed, None, batch_pairs, workspace_bytes,
                               num_threads)
    gt, gt_info = _entries(f1, f2, trans, o["ratio"], o["info"], len(clouds), min_ratio)
    return gt, gt_info, dict(frag1=f1, frag2=f2, trans=trans, ratio=o["ratio"], hits=o["hits"], info=o["info"],
                             kept=o["ratio"][:, 0] >= float(min_ratio))


# ------------------------------------------------------------------------------------------------ files
def read_fragment_pose(path) -> np.ndarray:
    """cloud_bin_<i>.info.txt -> the fragment's camera-to-world pose f64 [4,4]: rows 1 .. 4, columns 0 .. 3 of the file, as
    getGtInfoLog.m's dlmread(path, '\\t', [1, 0, 4, 3]) (row 0 is the scene's name and frame range)."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines()]
    if len(lines) < 5:
        raise ValueError("read_fragment_pose: %s has %d lines, 5 are needed" % (path, len(lines)))
    rows = [[float(v) for v in ln.split()[:4]] for ln in lines[1:5]]
    if any(len(r) != 4 for r in rows):
        raise ValueError("read_fragment_pose: %s does not hold a 4 x 4 matrix in rows 1 .. 4" % path)
    return np.array(rows, np.float64)


def write_fragment_pose(path, pose, scene: str = "scene", first: int = 0, last: int = 0):
    """The layout depth-fusion's fuseSceneFragments.m writes: `scene \\t first \\t last`, then the 4 x 4 row by row."""
    with open(path, "w") as f:
        f.write("%s\t %d\t %d\t\n" % (scene, first, last))
        for row in np.asarray(pose, np.float64).reshape(4, 4):
            f.write("%15.8e\t %15.8e\t %15.8e\t %15.8e\t\n" % tuple(row))


def write_scene_ground_truth(directory, gt: Sequence, gt_info: Sequence):
    """-> (directory/gt.log, directory/gt.info), through fragments.write_log and write_info."""
    os.makedirs(directory, exist_ok=True)
    log, info = os.path.join(directory, "gt.log"), os.path.join(directory, "gt.info")
    fragments.write_log(log, gt)
    fragments.write_info(info, gt_info)
    return log, info


# ------------------------------------------------------------------------------------------------ indoor repeatability
def repeatability_pairs(gt: Sequence) -> List[Tuple[int, int, np.ndarray]]:
    """build_3dmatch_dataset.m's list for one scene: (anchor fragment, positive fragment, T) per gt.log entry, in its order."""
    return [(int(g.info[0]), int(g.info[1]), np.asarray(g.trans, np.float64).reshape(4, 4)) for g in gt]


def _rep_batch(gt, kp_shape, count_shape):
    pairs = repeatability_pairs(gt)
    if len(kp_shape) != 3 or kp_shape[1] != 3 or tuple(count_shape) != (kp_shape[0],):
        raise ValueError("scene_repeatability: keypoints must be [F,3,M] with counts [F]")
    a = np.array([p[0] for p in pairs], np.int64)
    b = np.array([p[1] for p in pairs], np.int64)
    if len(pairs) and not (0 <= min(a.min(), b.min()) and max(a.max(), b.max()) < kp_shape[0]):
        raise ValueError("scene_repeatability: gt names a fragment outside 0 .. %d" % (kp_shape[0] - 1))
    T = np.ascontiguousarray(np.stack([p[2][:3] for p in pairs])) if pairs else np.zeros((0, 3, 4))
    return a, b, T


def scene_repeatability(kp, count, gt: Sequence, radius: float, pos_kp=None, pos_count=None):
    """eval_rep.m over build_3dmatch_dataset.m's pairs of one scene, on the device: kp f32 [F,3,M] and count i32 [F] (every
    fragment's keypoints; pos_kp, pos_count: another set for the positive side) -> (ratio f64 [E], hits i32 [E]) per gt.log
    entry: the share of the anchor fragment's keypoints whose nearest positive keypoint, moved by the entry's transform, is
    closer than radius (evaluation.repeatability, f-6's kernel).  No host synchronisation."""
    pos_kp, pos_count = (kp if pos_kp is None else pos_kp), (count if pos_count is None else pos_count)
    a, b, T = _rep_batch(gt, tuple(kp.shape), tuple(count.shape))
    if not len(a):
        return (torch.zeros((0,), dtype=torch.float64, device=kp.device), torch.zeros((0,), dtype=torch.int32, device=kp.device))
    ia, ib = torch.from_numpy(a).to(kp.device), torch.from_numpy(b).to(kp.device)
    ratio, hits, _ = evaluation.repeatability(kp[ia].contiguous(), count[ia].contiguous(), pos_kp[ib].contiguous(),
                                              pos_count[ib].contiguous(), torch.from_numpy(T).to(kp.device), radius)
    return ratio, hits


def scene_repeatability_cpu(kp, count, gt: Sequence, radius: float, pos_kp=None, pos_count=None):
    kp, count = np.asarray(kp, np.float32), np.asarray(count, np.int32)
    pos_kp = kp if pos_kp is None else np.asarray(pos_kp, np.float32)
    pos_count = count if pos_count is None else np.asarray(pos_count, np.int32)
    a, b, T = _rep_batch(gt, kp.shape, count.shape)
    if not len(a):
        return np.zeros(0), np.zeros(0, np.int32)
    ratio, hits, _ = evaluation.repeatability_cpu(kp[a], count[a], pos_kp[b], pos_count[b], T, radius)
    return ratio, hits
