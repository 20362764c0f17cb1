"""Baseline keypoint detectors on the device: what the reference compares its learned detector with.

evaluation/save_keypoints.py has method = 'tsf' | 'iss' | 'harris' | 'sift' | 'random'; the hand-crafted ones come from an
external PCL binding that is not part of the reference.  Here ISS (Intrinsic Shape Signatures, the parameters
save_keypoints.py:44-50 pins) and Harris3D (save_keypoints.py:52-55: radius 1, threshold 0.001) run as HIP kernels (csrc/iss.hip,
csrc/harris.hip; the definitions are in include/usip_hip.h, csrc/iss_math.h and csrc/harris_math.h), `random` and the rule that brings every method to the same keypoint count (ensure_keypoint_number,
save_keypoints.py:219-227, 326-331) are torch plumbing on the device:

    det = IssDetector(num=512, seed=0)                       # radii 2 / 2, gamma 0.975 / 0.975, min_neighbors 5
    kp, count = det(pc, count=None, frame_ids=[0, 1])        # pc f32 [B,3,N] on the device -> f32 [B,3,512], i32 [B]
    evaluator.add_frame_keypoints(fid, pc, sn, kp, count)    # evaluation.RegistrationEvaluator: score them
    det = HarrisDetector(num=512, seed=0)                    # radius 1, threshold 0.001, response "harris"

  iss_saliency       saliency f64 [B,N] and the neighbour counts at the salient radius
  iss_keypoints      (mask u8 [B,N], saliency, neighbours)
  harris_normals     normals f64 [B,3,N] over the radius and the neighbour counts; fewer than min_neighbors: no normal, zeros
  harris_response    (response f64 [B,N], members i32 [B,N], normals f64 [B,3,N]) from estimated or supplied normals
  harris_keypoints   (mask u8 [B,N], response, members, normals): at or above the threshold, no larger response in reach
  select_keypoints   mask -> exactly `num` keypoints per frame (or at most, with ensure=False)
  random_keypoints   `num` distinct points per frame
  *_cpu              the same on numpy arrays over the library's host twins (csrc/iss_cpu.cpp, csrc/harris_cpu.cpp)

The selection is reproducible and free of host synchronisation: one CPU generator per frame, seeded from (seed, frame_id) the
way prepare._keep_rows seeds its own, draws u in [0, 1) for every point; a live point's key is u when it is a keypoint and
1 + u otherwise, a dead slot's +inf; the first `num` points in ascending key (ties towards the lower index) are the frame's
keypoints.  With more than `num` keypoints that is a uniform subset, as the reference draws one; with fewer, every keypoint
comes first and uniform random cloud points pad.  The padding never repeats a keypoint -- the reference's np.random.choice
over the whole cloud could.  `random` gives every live point the key u.  SIFT3D is not built.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

ISS_DEFAULTS = dict(salient_radius=2.0, non_max_radius=2.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)
HARRIS_DEFAULTS = dict(radius=1.0, threshold=0.001, response="harris", min_neighbors=3)


def _check(salient_radius, non_max_radius, min_neighbors):
    if not (float(salient_radius) > 0.0 and float(non_max_radius) > 0.0 and int(min_neighbors) >= 1):
        raise ValueError("iss: the radii must be positive and min_neighbors at least 1")


def sort_along_x(pc: torch.Tensor, count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """perm i32 [B,N]: every frame's live points ascending along x, ties towards the lower index, dead slots behind them."""
    x = pc[:, 0, :] + 0.0                                              # (-0.0 -> +0.0: the two compare equal)
    if count is not None:
        dead = torch.arange(pc.shape[2], device=pc.device).unsqueeze(0) >= count.unsqueeze(1)
        x = x.masked_fill(dead, float("inf"))
    return torch.argsort(x, dim=1, stable=True).to(torch.int32)


def _frames(pc, count):
    if not isinstance(pc, torch.Tensor) or pc.dim() != 3 or pc.shape[1] != 3:
        raise ValueError("expected pc f32 [B,3,N] on the device")
    if count is not None:
        count = count.to(torch.int32).contiguous()
    return pc.contiguous(), count


def iss_saliency(pc, count=None, salient_radius: float = 2.0, gamma_21: float = 0.975, gamma_32: float = 0.975,
                 min_neighbors: int = 5, perm=None, want_visits: bool = False):
    """pc f32 [B,3,N], count i32 [B] -> (saliency f64 [B,N], neighbours i32 [B,N][, tiles_visited i32 [B,ceil(N/256)]])."""
    _check(salient_radius, 1.0, min_neighbors)
    pc, count = _frames(pc, count)
    perm = sort_along_x(pc, count) if perm is None else perm
    return ops.iss_saliency(pc, count, perm, salient_radius, gamma_21, gamma_32, min_neighbors, want_visits)


def iss_keypoints(pc, count=None, salient_radius: float = 2.0, non_max_radius: float = 2.0, gamma_21: float = 0.975,
                  gamma_32: float = 0.975, min_neighbors: int = 5):
    """-> (mask u8 [B,N], saliency f64 [B,N], neighbours i32 [B,N]).  No host synchronisation."""
    _check(salient_radius, non_max_radius, min_neighbors)
    pc, count = _frames(pc, count)
    perm = sort_along_x(pc, count)
    sal, nb = ops.iss_saliency(pc, count, perm, salient_radius, gamma_21, gamma_32, min_neighbors)
    return ops.iss_nms(pc, count, perm, sal, non_max_radius, min_neighbors), sal, nb


# ------------------------------------------------------------------------------------------------ Harris3D
def _check_harris(radius, threshold, response, min_neighbors):
    if not (0.0 < float(radius) < float("inf") and float(threshold) >= 0.0 and int(min_neighbors) >= 1):
        raise ValueError("harris: the radius must be positive and finite, the threshold at least 0 and min_neighbors at least 1")
    if response not in ops.HARRIS_METHODS:
        raise ValueError("harris: response must be one of %s, got %r" % (sorted(ops.HARRIS_METHODS), response))


def _supplied(normals, pc):
    """PCL's setNormals: f32 [B,3,N], used as given -- cast to float64, not renormalised"""
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or normals.shape != pc.shape \
            or normals.device != pc.device:
        raise ValueError("harris: supplied normals must be f32 %s on %s" % (tuple(pc.shape), pc.device))
    return normals.to(torch.float64).contiguous()


def harris_normals(pc, count=None, radius: float = 1.0, min_neighbors: int = 3, perm=None):
    """pc f32 [B,3,N], count i32 [B] -> (normals f64 [B,3,N], neighbours i32 [B,N])."""
    _check_harris(radius, 0.0, "harris", min_neighbors)
    pc, count = _frames(pc, count)
    perm = sort_along_x(pc, count) if perm is None else perm
    return ops.harris_normals(pc, count, perm, radius, min_neighbors)


def harris_response(pc, count=None, radius: float = 1.0, normals=None, response: str = "harris", min_neighbors: int = 3,
                    perm=None, want_visits: bool = False):
    """pc f32 [B,3,N], count i32 [B], normals f32 [B,3,N] or None (estimated over the radius) -> (response f64 [B,N], members
    i32 [B,N], normals f64 [B,3,N][, tiles_visited i32 [B,ceil(N/256)]])."""
    _check_harris(radius, 0.0, response, min_neighbors)
    pc, count = _frames(pc, count)
    perm = sort_along_x(pc, count) if perm is None else perm
    nrm = ops.harris_normals(pc, count, perm, radius, min_neighbors)[0] if normals is None else _supplied(normals, pc)
    out = ops.harris_response(pc, count, perm, nrm, radius, response, want_visits)
    return out[:2] + (nrm,) + out[2:]


def harris_keypoints(pc, count=None, radius: float = 1.0, threshold: float = 0.001, normals=None, response: str = "harris",
                     min_neighbors: int = 3):
    """-> (mask u8 [B,N], response f64 [B,N], members i32 [B,N], normals f64 [B,3,N]).  One sort, no host synchronisation."""
    _check_harris(radius, threshold, response, min_neighbors)
    pc, count = _frames(pc, count)
    perm = sort_along_x(pc, count)
    res, members, nrm = harris_response(pc, count, radius, normals, response, min_neighbors, perm)
    kept = torch.where(res >= float(threshold), res, torch.zeros_like(res))
    return ops.iss_nms(pc, count, perm, kept, radius, 1), res, members, nrm


# ------------------------------------------------------------------------------------------------ the selection rule
def _draws(B: int, N: int, seed: int, frame_ids: Optional[Sequence[int]]) -> torch.Tensor:
    """u f64 [B,N] on the host: frame b's row from a generator seeded by (seed, frame_ids[b])."""
    ids = list(range(B)) if frame_ids is None else [int(i) for i in frame_ids]
    if len(ids) != B:
        raise ValueError("frame_ids must name every frame of the batch (%d), got %d" % (B, len(ids)))
    u = torch.empty((B, N), dtype=torch.float64)
    for b, fid in enumerate(ids):
        g = torch.Generator(device="cpu")
        g.manual_seed((int(seed) * 1000003 + fid) & 0x7FFFFFFFFFFFFFFF)
        u[b] = torch.rand(N, generator=g, dtype=torch.float64)
    return u


def _select(pc, mask, count, num, ensure, u):
    """The rule on tensors of one device (the device path and, on host tensors, the twin)."""
    B, _, N = pc.shape
    num = int(num)
    if num < 1:
        raise ValueError("num must be at least 1")
    live = torch.ones((B, N), dtype=torch.bool, device=pc.device) if count is None else \
        torch.arange(N, device=pc.device).unsqueeze(0) < count.unsqueeze(1)
    is_kp = live if mask is None else (mask.to(torch.bool) & live)
    key = torch.where(is_kp, u, u + 1.0).masked_fill(~live, float("inf"))
    order = torch.argsort(key, dim=1, stable=True)[:, :num]
    lives = live.sum(1)
    if ensure or mask is None:
        cnt = torch.clamp(lives, max=num)
    else:
        found = is_kp.sum(1)
        none = found == 0                                              # save_keypoints.py:355-356: the frame's point 0
        order = torch.cat((torch.where(none.unsqueeze(1), torch.zeros_like(order[:, :1]), order[:, :1]), order[:, 1:]), 1)
        cnt = torch.where(none, torch.ones_like(found), torch.clamp(found, max=num))
    if order.shape[1] < num:
        order = torch.cat((order, order[:, :1].expand(-1, num - order.shape[1])), 1)
    slot = torch.arange(num, device=pc.device).unsqueeze(0)
    order = torch.where(slot < cnt.unsqueeze(1), order, order[:, :1])  # the slots beyond count hold the first pick
    kp = torch.gather(pc, 2, order.unsqueeze(1).expand(-1, 3, -1)).contiguous()
    return kp, cnt.to(torch.int32), order


def select_keypoints(pc, mask, count, num: int, ensure: bool = True, seed: int = 0, frame_ids=None, want_index: bool = False):
    """pc f32 [B,3,N], mask u8 [B,N], count i32 [B] or None -> (kp f32 [B,3,num], count i32 [B]): exactly min(num, live
    points) keypoints per frame with ensure, else min(num, keypoints found) -- the frame's point 0 when none was found.  The
    slots beyond count hold the frame's first pick.  want_index: also the picked point indices i64 [B,num]."""
    pc, count = _frames(pc, count)
    u = _draws(pc.shape[0], pc.shape[2], seed, frame_ids).to(pc.device, non_blocking=True)
    kp, cnt, order = _select(pc, mask, count, num, ensure, u)
    return (kp, cnt, order) if want_index else (kp, cnt)


def random_keypoints(pc, count, num: int, seed: int = 0, frame_ids=None, want_index: bool = False):
    """method = 'random' (save_keypoints.py:326-331): `num` distinct live points per frame, uniformly."""
    pc, count = _frames(pc, count)
    u = _draws(pc.shape[0], pc.shape[2], seed, frame_ids).to(pc.device, non_blocking=True)
    kp, cnt, order = _select(pc, None, count, num, True, u)
    return (kp, cnt, order) if want_index else (kp, cnt)


class IssDetector:
    """ISS with its parameters and the keypoint count bundled: __call__(pc, count, frame_ids) -> (kp f32 [B,3,num], count
    i32 [B]); .last holds (mask, saliency, neighbours) of the latest call."""

    def __init__(self, num: int = 512, ensure: bool = True, seed: int = 0, salient_radius: float = 2.0,
                 non_max_radius: float = 2.0, gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5):
        _check(salient_radius, non_max_radius, min_neighbors)
        self.num, self.ensure, self.seed = int(num), bool(ensure), int(seed)
        self.params = dict(salient_radius=float(salient_radius), non_max_radius=float(non_max_radius),
                           gamma_21=float(gamma_21), gamma_32=float(gamma_32), min_neighbors=int(min_neighbors))
        self.last = None

    def __call__(self, pc, count=None, frame_ids=None) -> Tuple[torch.Tensor, torch.Tensor]:
        self.last = iss_keypoints(pc, count, **self.params)
        return select_keypoints(pc, self.last[0], count, self.num, self.ensure, self.seed, frame_ids)


class HarrisDetector:
    """Harris3D with its parameters and the keypoint count bundled: __call__(pc, count, frame_ids) -> (kp f32 [B,3,num], count
    i32 [B]); .last holds (mask, response, members, normals) of the latest call."""

    def __init__(self, num: int = 512, ensure: bool = True, seed: int = 0, radius: float = 1.0, threshold: float = 0.001,
                 response: str = "harris"):
        _check_harris(radius, threshold, response, 3)
        self.num, self.ensure, self.seed = int(num), bool(ensure), int(seed)
        self.params = dict(radius=float(radius), threshold=float(threshold), response=response)
        self.last = None

    def __call__(self, pc, count=None, frame_ids=None) -> Tuple[torch.Tensor, torch.Tensor]:
        self.last = harris_keypoints(pc, count, **self.params)
        return select_keypoints(pc, self.last[0], count, self.num, self.ensure, self.seed, frame_ids)


# ------------------------------------------------------------------------------------------------ host twins (numpy)
def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _frames_np(pc, count):
    a = np.ascontiguousarray(pc, dtype=np.float32)
    if a.ndim != 3 or a.shape[1] != 3:
        raise ValueError("expected pc f32 [B,3,N], got %s" % (a.shape,))
    c = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
    if c is not None and c.shape != (a.shape[0],):
        raise ValueError("count must be i32 [B]")
    return a, c


def iss_saliency_cpu(pc, count=None, salient_radius: float = 2.0, gamma_21: float = 0.975, gamma_32: float = 0.975,
                     min_neighbors: int = 5, num_threads: int = 1):
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    sal, nb = np.zeros((B, N), np.float64), np.zeros((B, N), np.int32)
    _lib.check(_lib.lib().usip_iss_saliency_f32_cpu(_p(a), _p(c), B, N, float(salient_radius), float(gamma_21),
                                                    float(gamma_32), int(min_neighbors), _p(sal), _p(nb), int(num_threads)),
               "usip_iss_saliency_f32_cpu")
    return sal, nb


def iss_keypoints_cpu(pc, count=None, salient_radius: float = 2.0, non_max_radius: float = 2.0, gamma_21: float = 0.975,
                      gamma_32: float = 0.975, min_neighbors: int = 5, num_threads: int = 1):
    """-> (mask u8 [B,N], saliency f64 [B,N], neighbours i32 [B,N])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    sal, nb = iss_saliency_cpu(a, c, salient_radius, gamma_21, gamma_32, min_neighbors, num_threads)
    mask = np.zeros((B, N), np.uint8)
    _lib.check(_lib.lib().usip_iss_nms_f32_cpu(_p(a), _p(c), _p(sal), B, N, float(non_max_radius), int(min_neighbors),
                                               _p(mask), int(num_threads)), "usip_iss_nms_f32_cpu")
    return mask, sal, nb


def harris_normals_cpu(pc, count=None, radius: float = 1.0, min_neighbors: int = 3, num_threads: int = 1):
    """-> (normals f64 [B,3,N], neighbours i32 [B,N])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    nrm, nb = np.zeros((B, 3, N), np.float64), np.zeros((B, N), np.int32)
    _lib.check(_lib.lib().usip_harris_normals_f32_cpu(_p(a), _p(c), B, N, float(radius), int(min_neighbors), _p(nrm), _p(nb),
                                                      int(num_threads)), "usip_harris_normals_f32_cpu")
    return nrm, nb


def harris_response_cpu(pc, count=None, radius: float = 1.0, normals=None, response: str = "harris", min_neighbors: int = 3,
                        num_threads: int = 1):
    """-> (response f64 [B,N], members i32 [B,N], normals f64 [B,3,N])"""
    _check_harris(radius, 0.0, response, min_neighbors)
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    if normals is None:
        nrm = harris_normals_cpu(a, c, radius, min_neighbors, num_threads)[0]
    else:
        nrm = np.asarray(normals)
        if nrm.dtype != np.float32 or nrm.shape != a.shape:
            raise ValueError("harris: supplied normals must be f32 %s" % (a.shape,))
        nrm = np.ascontiguousarray(nrm, dtype=np.float64)
    res, members = np.zeros((B, N), np.float64), np.zeros((B, N), np.int32)
    _lib.check(_lib.lib().usip_harris_response_f32_cpu(_p(a), _p(c), _p(nrm), B, N, float(radius),
                                                       ops.HARRIS_METHODS[response], _p(res), _p(members), int(num_threads)),
               "usip_harris_response_f32_cpu")
    return res, members, nrm


def harris_keypoints_cpu(pc, count=None, radius: float = 1.0, threshold: float = 0.001, normals=None,
                         response: str = "harris", min_neighbors: int = 3, num_threads: int = 1):
    """-> (mask u8 [B,N], response f64 [B,N], members i32 [B,N], normals f64 [B,3,N])"""
    _check_harris(radius, threshold, response, min_neighbors)
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    res, members, nrm = harris_response_cpu(a, c, radius, normals, response, min_neighbors, num_threads)
    kept = np.where(res >= float(threshold), res, 0.0)
    mask = np.zeros((B, N), np.uint8)
    _lib.check(_lib.lib().usip_iss_nms_f32_cpu(_p(a), _p(c), _p(kept), B, N, float(radius), 1, _p(mask), int(num_threads)),
               "usip_iss_nms_f32_cpu")
    return mask, res, members, nrm


def _select_cpu(pc, mask, count, num, ensure, seed, frame_ids, want_index):
    a, c = _frames_np(pc, count)
    u = _draws(a.shape[0], a.shape[2], seed, frame_ids)
    kp, cnt, order = _select(torch.from_numpy(a), None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)),
                             None if c is None else torch.from_numpy(c), num, ensure, u)
    return (kp.numpy(), cnt.numpy(), order.numpy()) if want_index else (kp.numpy(), cnt.numpy())


def select_keypoints_cpu(pc, mask, count, num: int, ensure: bool = True, seed: int = 0, frame_ids=None,
                         want_index: bool = False):
    return _select_cpu(pc, mask, count, num, ensure, seed, frame_ids, want_index)


def random_keypoints_cpu(pc, count, num: int, seed: int = 0, frame_ids=None, want_index: bool = False):
    return _select_cpu(pc, None, count, num, True, seed, frame_ids, want_index)
