"""Baseline keypoint detectors on the device: what the reference compares its learned detector with.

evaluation/save_keypoints.py has method = 'tsf' | 'iss' | 'harris' | 'sift' | 'random'; the hand-crafted ones come from an
external PCL binding that is not part of the reference.  Here ISS (Intrinsic Shape Signatures, the parameters
save_keypoints.py:44-50 pins) and Harris3D (save_keypoints.py:52-55: radius 1, threshold 0.001) run as HIP kernels (csrc/iss.hip,
csrc/harris.hip; the definitions are in include/usip_hip.h, csrc/iss_math.h and csrc/harris_math.h), `random` and the rule that brings every method to the same keypoint count (ensure_keypoint_number,
save_keypoints.py:219-227, 326-331) are torch plumbing on the device.  SIFT3D (save_keypoints.py:57-61: min_scale 0.5, 4 octaves,
8 scales per octave, min_contrast 0.1; csrc/sift.hip, csrc/sift_math.h) runs over a scalar field of the cloud -- the
binding receives nothing but xyz, so the field is an axis ("z" by default, PCL's selector for xyz-only clouds) or an f32 [B,N]
tensor of the caller's (curvature, reflectance); its keypoints are voxel-cell centroids, not cloud points:

    det = IssDetector(num=512, seed=0)                       # radii 2 / 2, gamma 0.975 / 0.975, min_neighbors 5
    kp, count = det(pc, count=None, frame_ids=[0, 1])        # pc f32 [B,3,N] on the device -> f32 [B,3,512], i32 [B]
    evaluator.add_frame_keypoints(fid, pc, sn, kp, count)    # evaluation.RegistrationEvaluator: score them
    det = HarrisDetector(num=512, seed=0)                    # radius 1, threshold 0.001, response "harris"
    det = SiftDetector(num=512, seed=0)                      # min_scale 0.5, 4 octaves, 8 scales, min_contrast 0.1, field "z"

  iss_saliency       saliency f64 [B,N] and the neighbour counts at the salient radius
  iss_keypoints      (mask u8 [B,N], saliency, neighbours)
  harris_normals     normals f64 [B,3,N] over the radius and the neighbour counts; fewer than min_neighbors: no normal, zeros
  harris_response    (response f64 [B,N], members i32 [B,N], normals f64 [B,3,N]) from estimated or supplied normals
  harris_keypoints   (mask u8 [B,N], response, members, normals): at or above the threshold, no larger response in reach
  sift_octave        the voxel average of a cloud and its field at a leaf: (cloud f32 [B,3,N], field f32 [B,N], count i32 [B])
  sift_scale_space   dog f64 [B,S-1,N] of an octave cloud: differences of the Gaussian-smoothed field over S scales
  sift_keypoints     (candidates f32 [B,3,O*N], mask u8 [B,O*N], scale f64 [B,O*N], octave_count i32 [B,O]) over all octaves
  select_candidates  SIFT's candidates (and, with ensure, the cloud's points behind them) -> `num` keypoints per frame
  select_keypoints   mask -> exactly `num` keypoints per frame (or at most, with ensure=False)
  random_keypoints   `num` distinct points per frame
  fpfh_spfh          (spfh i32 [B,N,33], members i32 [B,N], normals f64 [B,3,N]): every point's integer pair-feature histograms
  fpfh_descriptors   (desc f32 [B,33,M], kp_members i32 [B,M]) at keypoints f32 [B,3,M] of any detector: FPFH
  shot_frames        (lrf f64 [B,M,9], lrf_members i32 [B,M]): every keypoint's local reference frame, zeros without one
  shot_descriptors   (desc f32 [B,352,M], kp_members i32 [B,M]) at keypoints f32 [B,3,M] of any detector: SHOT
  spin_descriptors   (desc f32 [B,153,M], kp_members i32 [B,M]) at keypoints f32 [B,3,M] of any detector: spin images
  *_cpu              the same on numpy arrays over the library's host twins (csrc/iss_cpu.cpp, csrc/harris_cpu.cpp,
                     csrc/sift_cpu.cpp, csrc/fpfh_cpu.cpp, csrc/shot_cpu.cpp, csrc/spin_cpu.cpp)

The scoring scripts of the reference also name hand-crafted DESCRIPTORS (eval_indoor/3dmatch/evaluate.m: 'my'; % 3dmatch, spin,
fpfh) that it does not contain.  FPFH (csrc/fpfh.hip, csrc/fpfh_math.h) describes the keypoints of any detector above without a
network or a checkpoint:

    fpfh = FpfhDescriptor(radius=2.0, normal_radius=1.0)     # this project's radii: the reference gives none
    desc = fpfh(pc, kp, count, kp_count)                     # f32 [B,33,M]
    evaluator.add_frame_descriptors(fid, kp, desc, kp_count) # evaluation.RegistrationEvaluator: score them

The outdoor scoring script is set to SHOT (eval_outdoor/kitti/evaluate_kitti.m: .../kitti/shot/iss_256, FEATURE_DIM = 352);
ShotDescriptor (csrc/shot.hip, csrc/shot_math.h) is called the same way and gives f32 [B,352,M].  SpinDescriptor (csrc/spin.hip,
csrc/spin_math.h) is the `spin` of evaluate.m's comment: f32 [B,153,M], about the z axis of SHOT's local reference frame.

The selection is reproducible and free of host synchronisation: one CPU generator per frame, seeded from (seed, frame_id) the
way prepare._keep_rows seeds its own, draws u in [0, 1) for every point; a live point's key is u when it is a keypoint and
1 + u otherwise, a dead slot's +inf; the first `num` points in ascending key (ties towards the lower index) are the frame's
keypoints.  With more than `num` keypoints that is a uniform subset, as the reference draws one; with fewer, every keypoint
comes first and uniform random cloud points pad.  The padding never repeats a keypoint -- the reference's np.random.choice
over the whole cloud could.  `random` gives every live point the key u.  SIFT's candidates are not cloud points: select_candidates draws u for the O * N
candidate slots and the N cloud points of a frame from the same generator; a candidate keypoint's key is u, with ensure a live
cloud point's is 1 + u, everything else +inf.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

ISS_DEFAULTS = dict(salient_radius=2.0, non_max_radius=2.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)
HARRIS_DEFAULTS = dict(radius=1.0, threshold=0.001, response="harris", min_neighbors=3)
SIFT_DEFAULTS = dict(min_scale=0.5, n_octaves=4, n_scales_per_octave=8, min_contrast=0.1, field="z")
FPFH_DEFAULTS = dict(radius=2.0, normal_radius=1.0, min_neighbors=3)   # this project's choice: the reference gives none
SHOT_DEFAULTS = dict(radius=2.0, normal_radius=1.0, min_neighbors=3)   # this project's choice too
SPIN_DEFAULTS = dict(radius=2.0, axis_radius=None, support_angle_cos=0.0, normal_radius=1.0, min_neighbors=3,
                     structure="rectangular")                          # likewise; axis_radius None: the radius


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


def _normals_for(pc, count, perm, normals, radius, min_neighbors, tag):
    """normals f64 [B,3,N]: estimated over `radius` (harris_normals), or the supplied f32 [B,3,N] used as given (PCL's
    setNormals) -- cast to float64, not renormalised"""
    if normals is None:
        return ops.harris_normals(pc, count, perm, radius, min_neighbors)[0]
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or normals.shape != pc.shape \
            or normals.device != pc.device:
        raise ValueError("%s: supplied normals must be f32 %s on %s" % (tag, tuple(pc.shape), pc.device))
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
    nrm = _normals_for(pc, count, perm, normals, radius, min_neighbors, "harris")
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


# ------------------------------------------------------------------------------------------------ FPFH
def _check_radii(radius, normal_radius, min_neighbors, tag):
    if not (0.0 < float(radius) < float("inf") and 0.0 < float(normal_radius) < float("inf") and int(min_neighbors) >= 1):
        raise ValueError("%s: the radii must be positive and finite and min_neighbors at least 1" % tag)


def _keypoints(keypoints, kp_count, pc, tag):
    if not isinstance(keypoints, torch.Tensor) or keypoints.dim() != 3 or keypoints.shape[:2] != pc.shape[:2] \
            or keypoints.dtype != torch.float32 or keypoints.device != pc.device:
        raise ValueError("%s: expected keypoints f32 [B,3,M] beside the cloud" % tag)
    if not 1 <= keypoints.shape[2] <= ops.FPFH_MMAX:
        raise ValueError("%s: M must be in 1..%d, got %d" % (tag, ops.FPFH_MMAX, keypoints.shape[2]))
    return keypoints.contiguous(), None if kp_count is None else kp_count.to(torch.int32).contiguous()


def _channels_first(rows, kp_members, want_f64, *more):
    """a descriptor's f64 [B,M,W] rows -> (desc f32 [B,W,M], the layout the learned descriptor has, kp_members[, rows, *more]);
    tensors or numpy arrays"""
    if isinstance(rows, torch.Tensor):
        desc = rows.to(torch.float32).transpose(1, 2).contiguous()
    else:
        desc = np.ascontiguousarray(rows.astype(np.float32).transpose(0, 2, 1))
    return (desc, kp_members, rows) + more if want_f64 else (desc, kp_members)


def fpfh_spfh(pc, count=None, radius: float = 2.0, normals=None, normal_radius: float = 1.0, min_neighbors: int = 3,
              perm=None, want_visits: bool = False):
    """pc f32 [B,3,N], count i32 [B], normals f32 [B,3,N] or None (harris_normals over normal_radius with min_neighbors) ->
    (spfh i32 [B,N,33], members i32 [B,N], normals f64 [B,3,N][, tiles_visited i32 [B,ceil(N/256)]]): the integer counts of
    the three 11-bin pair-feature histograms of every point over its members within `radius`.  radius 2 and normal_radius 1
    (outdoor metres) are this project's choice: the reference gives none; indoor callers pass their own."""
    _check_radii(radius, normal_radius, min_neighbors, "fpfh")
    pc, count = _frames(pc, count)
    perm = sort_along_x(pc, count) if perm is None else perm
    nrm = _normals_for(pc, count, perm, normals, normal_radius, min_neighbors, "fpfh")
    out = ops.fpfh_spfh(pc, count, perm, nrm, radius, want_visits)
    return out[:2] + (nrm,) + out[2:]


def fpfh_descriptors(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, normals=None, normal_radius: float = 1.0,
                     want_f64: bool = False, min_neighbors: int = 3):
    """pc f32 [B,3,N], keypoints f32 [B,3,M] (any positions: cloud points or not), count, kp_count i32 [B] or None -> (desc f32
    [B,33,M], kp_members i32 [B,M][, fpfh f64 [B,M,33]]): Fast Point Feature Histograms at the keypoints, the layout the learned
    descriptor has (channels first).  The f32 descriptor is the cast of the f64 result.  One sort, no host synchronisation.
    radius 2 and normal_radius 1 are this project's choice (fpfh_spfh)."""
    _check_radii(radius, normal_radius, min_neighbors, "fpfh")
    pc, count = _frames(pc, count)
    keypoints, kp_count = _keypoints(keypoints, kp_count, pc, "fpfh")
    perm = sort_along_x(pc, count)
    spfh, members, _ = fpfh_spfh(pc, count, radius, normals, normal_radius, min_neighbors, perm)
    fpfh, kp_members = ops.fpfh_gather(pc, count, perm, spfh, members, keypoints, kp_count, radius)
    return _channels_first(fpfh, kp_members, want_f64)


# ------------------------------------------------------------------------------------------------ SHOT
def shot_frames(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, perm=None):
    """pc f32 [B,3,N], keypoints f32 [B,3,M] (any positions), count, kp_count i32 [B] or None -> (lrf f64 [B,M,9], lrf_members
    i32 [B,M]): the rows x, y, z of every keypoint's local reference frame over the live points within `radius`; zeros where
    there is none (fewer than 5 members)."""
    _check_radii(radius, 1.0, 1, "shot")
    pc, count = _frames(pc, count)
    keypoints, kp_count = _keypoints(keypoints, kp_count, pc, "shot")
    perm = sort_along_x(pc, count) if perm is None else perm
    return ops.shot_lrf(pc, count, perm, keypoints, kp_count, radius)


def shot_descriptors(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, normals=None, normal_radius: float = 1.0,
                     want_f64: bool = False, min_neighbors: int = 3):
    """pc f32 [B,3,N], keypoints f32 [B,3,M] (any positions: cloud points or not), count, kp_count i32 [B] or None, normals f32
    [B,3,N] or None (harris_normals over normal_radius with min_neighbors) -> (desc f32 [B,352,M], kp_members i32 [B,M][, shot
    f64 [B,M,352], hist i64 [B,M,352], lrf f64 [B,M,9], lrf_members i32 [B,M]]): SHOT-352 at the keypoints, the layout the
    learned descriptor has (channels first).  The f32 descriptor is the cast of the f64 result.  One sort, no host
    synchronisation.  radius 2 and normal_radius 1 (outdoor metres) are this project's choice: the reference gives none."""
    _check_radii(radius, normal_radius, min_neighbors, "shot")
    pc, count = _frames(pc, count)
    keypoints, kp_count = _keypoints(keypoints, kp_count, pc, "shot")
    perm = sort_along_x(pc, count)
    nrm = _normals_for(pc, count, perm, normals, normal_radius, min_neighbors, "shot")
    lrf, lrf_members = ops.shot_lrf(pc, count, perm, keypoints, kp_count, radius)
    hist, shot, kp_members = ops.shot_hist(pc, count, perm, nrm, keypoints, kp_count, lrf, radius)
    return _channels_first(shot, kp_members, want_f64, hist, lrf, lrf_members)


# ------------------------------------------------------------------------------------------------ spin images
def _check_spin(radius, axis_radius, support_angle_cos, normal_radius, min_neighbors, structure):
    _check_radii(radius, normal_radius, min_neighbors, "spin")
    if axis_radius is not None:
        _check_radii(axis_radius, 1.0, 1, "spin")
    if not 0.0 <= float(support_angle_cos) <= 1.0:
        raise ValueError("spin: support_angle_cos must be in [0, 1], got %r" % (support_angle_cos,))
    if structure not in ops.SPIN_STRUCTURES:
        raise ValueError("spin: structure must be one of %s, got %r" % (sorted(ops.SPIN_STRUCTURES), structure))


def spin_descriptors(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, axes=None, axis_radius=None,
                     support_angle_cos: float = 0.0, normals=None, normal_radius: float = 1.0, want_f64: bool = False,
                     min_neighbors: int = 3, structure: str = "rectangular"):
    """pc f32 [B,3,N], keypoints f32 [B,3,M] (any positions: cloud points or not), count, kp_count i32 [B] or None -> (desc f32
    [B,153,M], kp_members i32 [B,M][, spin f64 [B,M,153], hist i64 [B,M,153], axes f64 [B,M,3], lrf_members i32 [B,M] or
    None]): spin images at the keypoints, 9 rows of the distance from the axis by 17 columns of the height along it, the layout
    the learned descriptor has (channels first).  axes f64 [B,M,3] or None: the z row of shot_frames over axis_radius (None:
    radius), so a keypoint with fewer than 5 points there has no descriptor; supplied axes (normals oriented to the sensor,
    say) need not be of unit length.  support_angle_cos s > 0 keeps the members whose normal has |n . axis| >= s: normals f32
    [B,3,N] or None (harris_normals over normal_radius with min_neighbors); with s == 0 no normal is estimated or read.
    structure "rectangular" (the cylinder inscribed in the sphere) or "radial" (distance by elevation).  The f32 descriptor is
    the cast of the f64 result.  One sort, no host synchronisation.  The radii (outdoor metres) are this project's choice."""
    _check_spin(radius, axis_radius, support_angle_cos, normal_radius, min_neighbors, structure)
    pc, count = _frames(pc, count)
    keypoints, kp_count = _keypoints(keypoints, kp_count, pc, "spin")
    perm = sort_along_x(pc, count)
    nrm = None
    if float(support_angle_cos) > 0.0:
        nrm = _normals_for(pc, count, perm, normals, normal_radius, min_neighbors, "spin")
    lrf_members = None
    if axes is None:
        lrf, lrf_members = ops.shot_lrf(pc, count, perm, keypoints, kp_count, radius if axis_radius is None else axis_radius)
        axes = lrf[:, :, 6:9].contiguous()
    elif not isinstance(axes, torch.Tensor) or axes.dtype != torch.float64 or axes.device != pc.device \
            or tuple(axes.shape) != (pc.shape[0], keypoints.shape[2], 3):
        raise ValueError("spin: supplied axes must be f64 [B,M,3] on %s" % (pc.device,))
    else:
        axes = axes.contiguous()
    hist, spin, kp_members = ops.spin_image(pc, count, perm, nrm, keypoints, kp_count, axes, radius, support_angle_cos, structure)
    return _channels_first(spin, kp_members, want_f64, hist, axes, lrf_members)


# ------------------------------------------------------------------------------------------------ SIFT3D
_AXES = {"x": 0, "y": 1, "z": 2}


def _check_sift(min_scale, n_octaves, n_scales_per_octave, min_contrast):
    if not (0.0 < float(min_scale) < float("inf") and float(min_contrast) >= 0.0):
        raise ValueError("sift: min_scale must be positive and finite and min_contrast at least 0")
    if not (1 <= int(n_octaves) <= 8 and 1 <= int(n_scales_per_octave) <= 8):
        raise ValueError("sift: n_octaves and n_scales_per_octave must be in 1..8")


def _field(field, shape, like):
    """-> (axis, None) for "x" | "y" | "z", (0, the tensor / array) for a supplied f32 [B,N] field"""
    if isinstance(field, str):
        if field not in _AXES:
            raise ValueError("sift: field must be one of %s or f32 [B,N], got %r" % (sorted(_AXES), field))
        return _AXES[field], None
    if isinstance(like, torch.Tensor):
        ok = isinstance(field, torch.Tensor) and field.dtype == torch.float32 and field.device == like.device
    else:
        ok = isinstance(field, np.ndarray) and field.dtype == np.float32
    if not ok or tuple(field.shape) != tuple(shape):
        raise ValueError("sift: a supplied field must be f32 %s beside the cloud" % (tuple(shape),))
    return 0, field


def sift_sigma2(base: float, n_scales_per_octave: int) -> np.ndarray:
    """sigma_s^2 f64 [S] of the octave with base scale `base`: S = n_scales_per_octave + 3, sigma_s = base * 2^((s - 1) /
    n_scales_per_octave).  Computed once on the host; the kernel and the twin are handed this array."""
    k = int(n_scales_per_octave)
    sigma = np.float64(base) * np.power(np.float64(2.0), (np.arange(k + 3, dtype=np.float64) - 1.0) / np.float64(k))
    return sigma * sigma


def sift_walk_radius(sigma2) -> float:
    """the scale-space walk's radius: the smallest float64 r >= sqrt(9 sigma_{S-1}^2) with r * r >= 9 sigma_{S-1}^2"""
    t = np.float64(9.0) * np.float64(sigma2[-1])
    r = np.sqrt(t)
    while r * r < t:
        r = np.nextafter(r, np.inf)
    return float(r)


def sift_octave(pc, field="z", count=None, leaf: float = 0.5):
    """pc f32 [B,3,N], field "x" | "y" | "z" or f32 [B,N], count i32 [B] -> (cloud f32 [B,3,N], field f32 [B,N], count i32 [B]):
    one row per occupied cell of the grid of size `leaf` anchored at the origin, in ascending cell key; the row is the cell's
    centroid, its field the centroid's own coordinate (axis field) or the members' mean.  No host synchronisation."""
    pc, count = _frames(pc, count)
    axis, supplied = _field(field, (pc.shape[0], pc.shape[2]), pc)
    keys = ops.sift_voxel_keys(pc, count, leaf)
    sorted_keys, order = torch.sort(keys, dim=1, stable=True)
    return ops.sift_voxel_average(pc, None if supplied is None else supplied.contiguous(), axis, sorted_keys,
                                  order.to(torch.int32))


def sift_scale_space(cloud, field, count, base: float, n_scales_per_octave: int = 8, perm=None, want_visits: bool = False):
    """An octave cloud (sift_octave's three results) and its base scale -> dog f64 [B,S-1,N][, tiles_visited].  A frame with
    fewer than 25 points gets zeros."""
    _check_sift(base, 1, n_scales_per_octave, 0.0)
    cloud, count = _frames(cloud, count)
    perm = sort_along_x(cloud, count) if perm is None else perm
    return ops.sift_dog(cloud, field, count, perm, sift_sigma2(base, n_scales_per_octave), want_visits)


def sift_keypoints(pc, count=None, min_scale: float = 0.5, n_octaves: int = 4, n_scales_per_octave: int = 8,
                   min_contrast: float = 0.1, field="z", want_octaves: bool = False):
    """-> (candidates f32 [B,3,O*N], mask u8 [B,O*N], scale f64 [B,O*N], octave_count i32 [B,O]): octave o's cloud in slots o *
    N .. o * N + N, mask where a row is a keypoint, scale = sigma of the lowest scale at which it is extremal (0 elsewhere),
    octave_count the rows of every octave cloud.  No host synchronisation.  want_octaves: also the per-octave (cloud, field,
    count, dog, idx, mask, scale_index)."""
    _check_sift(min_scale, n_octaves, n_scales_per_octave, min_contrast)
    pc, count = _frames(pc, count)
    cloud, fld, cnt = pc, field, count
    clouds, masks, scales, counts, octaves = [], [], [], [], []
    for o in range(int(n_octaves)):
        base = float(min_scale) * 2.0 ** o
        cloud, fld, cnt = sift_octave(cloud, field if isinstance(field, str) else fld, cnt, base)
        perm = sort_along_x(cloud, cnt)
        sigma2 = sift_sigma2(base, n_scales_per_octave)
        dog = ops.sift_dog(cloud, fld, cnt, perm, sigma2)
        idx = ops.sift_nearest(cloud, cnt, perm)
        mask, sidx = ops.sift_extrema(dog, idx, cnt, min_contrast)
        sigma = torch.from_numpy(np.sqrt(sigma2)).to(pc.device, non_blocking=True)
        clouds.append(cloud)
        masks.append(mask)
        scales.append(torch.where(mask.to(torch.bool), sigma[sidx.long()], torch.zeros((), dtype=torch.float64, device=pc.device)))
        counts.append(cnt)
        octaves.append((cloud, fld, cnt, dog, idx, mask, sidx))
    out = (torch.cat(clouds, 2), torch.cat(masks, 1), torch.cat(scales, 1), torch.stack(counts, 1))
    return out + (octaves,) if want_octaves else out


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


def _take(points, order, cnt, num):
    """The tail of either rule: order i64 [B, <= num] padded to num, the slots beyond cnt hold the first pick -> (points f32
    [B,3,num] at order, cnt i32 [B], order)."""
    if order.shape[1] < num:
        order = torch.cat((order, order[:, :1].expand(-1, num - order.shape[1])), 1)
    slot = torch.arange(num, device=points.device).unsqueeze(0)
    order = torch.where(slot < cnt.unsqueeze(1), order, order[:, :1])
    kp = torch.gather(points, 2, order.unsqueeze(1).expand(-1, 3, -1)).contiguous()
    return kp, cnt.to(torch.int32), order


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
    return _take(pc, order, cnt, num)


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


def _select_candidates(pc, count, cand, mask, num, ensure, u):
    """SIFT's rule on tensors of one device: the slots are the M candidate slots, then the N cloud points."""
    B, _, N = pc.shape
    M = cand.shape[2]
    num = int(num)
    if num < 1:
        raise ValueError("num must be at least 1")
    live = torch.ones((B, N), dtype=torch.bool, device=pc.device) if count is None else \
        torch.arange(N, device=pc.device).unsqueeze(0) < count.unsqueeze(1)
    is_kp = mask.to(torch.bool)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=pc.device)
    key = torch.cat((torch.where(is_kp, u[:, :M], inf), torch.where(live, u[:, M:] + 1.0, inf) if ensure else
                     inf.expand(B, N)), 1)
    if not ensure:                                                      # save_keypoints.py:355-356: the frame's point 0
        key[:, M] = torch.where(is_kp.any(1), key[:, M], torch.zeros((), dtype=torch.float64, device=pc.device))
    order = torch.argsort(key, dim=1, stable=True)[:, :num]
    found = is_kp.sum(1)
    cnt = torch.clamp(found + live.sum(1), max=num) if ensure else \
        torch.where(found == 0, torch.ones_like(found), torch.clamp(found, max=num))
    return _take(torch.cat((cand, pc), 2), order, cnt, num)


def select_candidates(pc, count, candidates, mask, num: int, ensure: bool = True, seed: int = 0, frame_ids=None,
                      want_index: bool = False):
    """pc f32 [B,3,N], count i32 [B] or None, candidates f32 [B,3,M] with mask u8 [B,M] (sift_keypoints' first two results) ->
    (kp f32 [B,3,num], count i32 [B]).  One CPU generator per frame, seeded as select_keypoints seeds it, draws u for the M
    candidate slots and then the N cloud points; a candidate keypoint's key is u, with ensure a live cloud point's is 1 + u,
    everything else +inf; the first `num` in ascending key, ties towards the lower slot.  With ensure every keypoint comes
    first and uniform random cloud points pad to min(num, keypoints + live points); without, min(num, keypoints) -- the
    frame's point 0 with count 1 when none was found.  The slots beyond count hold the frame's first pick.  want_index: also
    the picked slots i64 [B,num] (below M a candidate slot, M + i the cloud's point i)."""
    pc, count = _frames(pc, count)
    M = candidates.shape[2]
    if candidates.shape[:2] != pc.shape[:2] or tuple(mask.shape) != (pc.shape[0], M):
        raise ValueError("expected candidates f32 [B,3,M] and mask u8 [B,M]")
    u = _draws(pc.shape[0], M + pc.shape[2], seed, frame_ids).to(pc.device, non_blocking=True)
    kp, cnt, order = _select_candidates(pc, count, candidates, mask, num, ensure, u)
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


class SiftDetector:
    """SIFT3D with its parameters and the keypoint count bundled: __call__(pc, count, frame_ids) -> (kp f32 [B,3,num], count
    i32 [B]); .last holds (candidates, mask, scale, octave_count) of the latest call.  field: "x" | "y" | "z"; a call may hand
    in a scalar of its own for its frames instead, field f32 [B,N]."""

    def __init__(self, num: int = 512, ensure: bool = True, seed: int = 0, min_scale: float = 0.5, n_octaves: int = 4,
                 n_scales_per_octave: int = 8, min_contrast: float = 0.1, field="z"):
        _check_sift(min_scale, n_octaves, n_scales_per_octave, min_contrast)
        if not isinstance(field, str) or field not in _AXES:
            raise ValueError("sift: field must be one of %s, got %r" % (sorted(_AXES), field))
        self.num, self.ensure, self.seed = int(num), bool(ensure), int(seed)
        self.params = dict(min_scale=float(min_scale), n_octaves=int(n_octaves), n_scales_per_octave=int(n_scales_per_octave),
                           min_contrast=float(min_contrast))
        self.field = field
        self.last = None

    def __call__(self, pc, count=None, frame_ids=None, field=None) -> Tuple[torch.Tensor, torch.Tensor]:
        self.last = sift_keypoints(pc, count, field=self.field if field is None else field, **self.params)
        return select_candidates(pc, count, self.last[0], self.last[1], self.num, self.ensure, self.seed, frame_ids)


class _Descriptor:
    """A descriptor (dim, describe) with its parameters bundled, called where the learned descriptor is"""

    def __init__(self, **params):
        self.params = params
        self.last = None

    def __call__(self, pc, keypoints, count=None, kp_count=None, normals=None) -> torch.Tensor:
        self.last = type(self).describe(pc, keypoints, count, kp_count, normals=normals, **self.params)
        return self.last[0]


class FpfhDescriptor(_Descriptor):
    """FPFH with its parameters bundled, called where the learned descriptor is: __call__(pc, keypoints, count, kp_count,
    normals) -> desc f32 [B,33,M]; .last holds (desc, kp_members) of the latest call.  normals f32 [B,3,N]: supplied ones (the
    cloud's sn[:, :3]) instead of estimated ones."""

    dim, describe = 33, staticmethod(fpfh_descriptors)

    def __init__(self, radius: float = 2.0, normal_radius: float = 1.0, min_neighbors: int = 3):
        _check_radii(radius, normal_radius, min_neighbors, "fpfh")
        super().__init__(radius=float(radius), normal_radius=float(normal_radius), min_neighbors=int(min_neighbors))


class ShotDescriptor(_Descriptor):
    """SHOT-352 with its parameters bundled, called where the learned descriptor is: __call__(pc, keypoints, count, kp_count,
    normals) -> desc f32 [B,352,M]; .last holds (desc, kp_members) of the latest call.  normals f32 [B,3,N]: supplied ones (the
    cloud's sn[:, :3]) instead of estimated ones."""

    dim, describe = 352, staticmethod(shot_descriptors)

    def __init__(self, radius: float = 2.0, normal_radius: float = 1.0, min_neighbors: int = 3):
        _check_radii(radius, normal_radius, min_neighbors, "shot")
        super().__init__(radius=float(radius), normal_radius=float(normal_radius), min_neighbors=int(min_neighbors))


class SpinDescriptor(_Descriptor):
    """Spin images with their parameters bundled, called where the learned descriptor is: __call__(pc, keypoints, count,
    kp_count, normals) -> desc f32 [B,153,M]; .last holds (desc, kp_members) of the latest call.  normals f32 [B,3,N]: supplied
    ones (the cloud's sn[:, :3]) instead of estimated ones, read only with a support angle."""

    dim, describe = 153, staticmethod(spin_descriptors)

    def __init__(self, radius: float = 2.0, axis_radius=None, support_angle_cos: float = 0.0, normal_radius: float = 1.0,
                 min_neighbors: int = 3, structure: str = "rectangular"):
        _check_spin(radius, axis_radius, support_angle_cos, normal_radius, min_neighbors, structure)
        super().__init__(radius=float(radius), axis_radius=None if axis_radius is None else float(axis_radius),
                         support_angle_cos=float(support_angle_cos), normal_radius=float(normal_radius),
                         min_neighbors=int(min_neighbors), structure=structure)


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


def _normals_for_np(a, c, normals, radius, min_neighbors, num_threads, tag):
    """_normals_for on numpy arrays: estimated by harris_normals_cpu, or the supplied f32 [B,3,N] cast to float64"""
    if normals is None:
        return harris_normals_cpu(a, c, radius, min_neighbors, num_threads)[0]
    nrm = np.asarray(normals)
    if nrm.dtype != np.float32 or nrm.shape != a.shape:
        raise ValueError("%s: supplied normals must be f32 %s" % (tag, a.shape))
    return np.ascontiguousarray(nrm, dtype=np.float64)


def _keypoints_np(keypoints, kp_count, B, tag):
    kp = np.ascontiguousarray(keypoints, dtype=np.float32)
    if kp.ndim != 3 or kp.shape[:2] != (B, 3):
        raise ValueError("%s: expected keypoints f32 [B,3,M], got %s" % (tag, kp.shape))
    kc = None if kp_count is None else np.ascontiguousarray(kp_count, dtype=np.int32)
    if kc is not None and kc.shape != (B,):
        raise ValueError("%s: kp_count must be i32 [B]" % tag)
    return kp, kc


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
    nrm = _normals_for_np(a, c, normals, radius, min_neighbors, num_threads, "harris")
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


def fpfh_spfh_cpu(pc, count=None, radius: float = 2.0, normals=None, normal_radius: float = 1.0, min_neighbors: int = 3,
                  num_threads: int = 1):
    """-> (spfh i32 [B,N,33], members i32 [B,N], normals f64 [B,3,N])"""
    _check_radii(radius, normal_radius, min_neighbors, "fpfh")
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    nrm = _normals_for_np(a, c, normals, normal_radius, min_neighbors, num_threads, "fpfh")
    spfh, members = np.zeros((B, N, ops.FPFH_WIDTH), np.int32), np.zeros((B, N), np.int32)
    _lib.check(_lib.lib().usip_fpfh_spfh_f32_cpu(_p(a), _p(c), _p(nrm), B, N, float(radius), _p(spfh), _p(members),
                                                 int(num_threads)), "usip_fpfh_spfh_f32_cpu")
    return spfh, members, nrm


def fpfh_gather_cpu(pc, count, spfh, members, keypoints, kp_count, radius: float, num_threads: int = 1):
    """-> (fpfh f64 [B,M,33], kp_members i32 [B,M])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    kp, kc = _keypoints_np(keypoints, kp_count, B, "fpfh")
    M = kp.shape[2]
    s, m = np.ascontiguousarray(spfh, dtype=np.int32), np.ascontiguousarray(members, dtype=np.int32)
    if s.shape != (B, N, ops.FPFH_WIDTH) or m.shape != (B, N):
        raise ValueError("fpfh: expected spfh i32 [B,N,33] and members i32 [B,N]")
    fpfh, kp_members = np.zeros((B, max(M, 1), ops.FPFH_WIDTH), np.float64), np.zeros((B, max(M, 1)), np.int32)
    _lib.check(_lib.lib().usip_fpfh_gather_f32_cpu(_p(a), _p(c), _p(s), _p(m), _p(kp), _p(kc), B, N, M, float(radius),
                                                   _p(fpfh), _p(kp_members), int(num_threads)), "usip_fpfh_gather_f32_cpu")
    return fpfh, kp_members


def fpfh_descriptors_cpu(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, normals=None,
                         normal_radius: float = 1.0, want_f64: bool = False, min_neighbors: int = 3, num_threads: int = 1):
    """-> (desc f32 [B,33,M], kp_members i32 [B,M][, fpfh f64 [B,M,33]])"""
    spfh, members, _ = fpfh_spfh_cpu(pc, count, radius, normals, normal_radius, min_neighbors, num_threads)
    fpfh, kp_members = fpfh_gather_cpu(pc, count, spfh, members, keypoints, kp_count, radius, num_threads)
    return _channels_first(fpfh, kp_members, want_f64)


def shot_frames_cpu(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, num_threads: int = 1):
    """-> (lrf f64 [B,M,9], lrf_members i32 [B,M])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    kp, kc = _keypoints_np(keypoints, kp_count, B, "shot")
    M = kp.shape[2]
    lrf, members = np.zeros((B, max(M, 1), 9), np.float64), np.zeros((B, max(M, 1)), np.int32)
    _lib.check(_lib.lib().usip_shot_lrf_f32_cpu(_p(a), _p(c), _p(kp), _p(kc), B, N, M, float(radius), _p(lrf), _p(members),
                                                int(num_threads)), "usip_shot_lrf_f32_cpu")
    return lrf, members


def shot_hist_cpu(pc, count, normals, keypoints, kp_count, lrf, radius: float, num_threads: int = 1):
    """normals f64 [B,3,N], lrf f64 [B,M,9] -> (hist i64 [B,M,352], shot f64 [B,M,352], kp_members i32 [B,M])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    kp, kc = _keypoints_np(keypoints, kp_count, B, "shot")
    M = kp.shape[2]
    nrm, frames = np.ascontiguousarray(normals, dtype=np.float64), np.ascontiguousarray(lrf, dtype=np.float64)
    if nrm.shape != a.shape or frames.shape != (B, M, 9):
        raise ValueError("shot: expected normals f64 [B,3,N] and lrf f64 [B,M,9]")
    hist, shot = np.zeros((B, max(M, 1), ops.SHOT_WIDTH), np.int64), np.zeros((B, max(M, 1), ops.SHOT_WIDTH), np.float64)
    kp_members = np.zeros((B, max(M, 1)), np.int32)
    _lib.check(_lib.lib().usip_shot_hist_f32_cpu(_p(a), _p(c), _p(nrm), _p(kp), _p(kc), _p(frames), B, N, M, float(radius),
                                                 _p(hist), _p(shot), _p(kp_members), int(num_threads)), "usip_shot_hist_f32_cpu")
    return hist, shot, kp_members


def shot_descriptors_cpu(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, normals=None,
                         normal_radius: float = 1.0, want_f64: bool = False, min_neighbors: int = 3, num_threads: int = 1):
    """-> (desc f32 [B,352,M], kp_members i32 [B,M][, shot f64 [B,M,352], hist i64 [B,M,352], lrf f64 [B,M,9], lrf_members i32
    [B,M]])"""
    _check_radii(radius, normal_radius, min_neighbors, "shot")
    a, c = _frames_np(pc, count)
    nrm = _normals_for_np(a, c, normals, normal_radius, min_neighbors, num_threads, "shot")
    lrf, lrf_members = shot_frames_cpu(a, keypoints, c, kp_count, radius, num_threads)
    hist, shot, kp_members = shot_hist_cpu(a, c, nrm, keypoints, kp_count, lrf, radius, num_threads)
    return _channels_first(shot, kp_members, want_f64, hist, lrf, lrf_members)


def shot_angle_cpu(y, x):
    """csrc/shot_math.h's inverse tangent of two arguments, as the kernels and the twin evaluate it"""
    a, b = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError("shot: y and x must have one shape")
    out = np.zeros_like(a)
    _lib.check(_lib.lib().usip_shot_angle_f64_cpu(_p(a), _p(b), a.size, _p(out)), "usip_shot_angle_f64_cpu")
    return out


def spin_image_cpu(pc, count, normals, keypoints, kp_count, axes, radius: float, support_angle_cos: float = 0.0,
                   structure: str = "rectangular", num_threads: int = 1):
    """normals f64 [B,3,N] or None, axes f64 [B,M,3] -> (hist i64 [B,M,153], spin f64 [B,M,153], kp_members i32 [B,M])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    kp, kc = _keypoints_np(keypoints, kp_count, B, "spin")
    M = kp.shape[2]
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    ax = np.ascontiguousarray(axes, dtype=np.float64)
    if (nrm is not None and nrm.shape != a.shape) or ax.shape != (B, M, 3):
        raise ValueError("spin: expected normals f64 [B,3,N] or None and axes f64 [B,M,3]")
    if structure not in ops.SPIN_STRUCTURES:
        raise ValueError("spin: structure must be one of %s, got %r" % (sorted(ops.SPIN_STRUCTURES), structure))
    hist, spin = np.zeros((B, max(M, 1), ops.SPIN_WIDTH), np.int64), np.zeros((B, max(M, 1), ops.SPIN_WIDTH), np.float64)
    kp_members = np.zeros((B, max(M, 1)), np.int32)
    _lib.check(_lib.lib().usip_spin_image_f32_cpu(_p(a), _p(c), _p(nrm), _p(kp), _p(kc), _p(ax), B, N, M, float(radius),
                                                  float(support_angle_cos), ops.SPIN_STRUCTURES[structure], _p(hist), _p(spin),
                                                  _p(kp_members), int(num_threads)), "usip_spin_image_f32_cpu")
    return hist, spin, kp_members


def spin_descriptors_cpu(pc, keypoints, count=None, kp_count=None, radius: float = 2.0, axes=None, axis_radius=None,
                         support_angle_cos: float = 0.0, normals=None, normal_radius: float = 1.0, want_f64: bool = False,
                         min_neighbors: int = 3, structure: str = "rectangular", num_threads: int = 1):
    """-> (desc f32 [B,153,M], kp_members i32 [B,M][, spin f64 [B,M,153], hist i64 [B,M,153], axes f64 [B,M,3], lrf_members i32
    [B,M] or None])"""
    _check_spin(radius, axis_radius, support_angle_cos, normal_radius, min_neighbors, structure)
    a, c = _frames_np(pc, count)
    nrm = None
    if float(support_angle_cos) > 0.0:
        nrm = _normals_for_np(a, c, normals, normal_radius, min_neighbors, num_threads, "spin")
    lrf_members = None
    if axes is None:
        lrf, lrf_members = shot_frames_cpu(a, keypoints, c, kp_count, radius if axis_radius is None else axis_radius,
                                           num_threads)
        axes = np.ascontiguousarray(lrf[:, :, 6:9])
    hist, spin, kp_members = spin_image_cpu(a, c, nrm, keypoints, kp_count, axes, radius, support_angle_cos, structure,
                                            num_threads)
    return _channels_first(spin, kp_members, want_f64, hist, np.ascontiguousarray(axes, dtype=np.float64), lrf_members)


def sift_exp_cpu(x):
    """csrc/sift_math.h's float64 exponential, as the kernels and the twin evaluate it"""
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(a)
    _lib.check(_lib.lib().usip_sift_exp_f64_cpu(_p(a), a.size, _p(out)), "usip_sift_exp_f64_cpu")
    return out


def sift_octave_cpu(pc, field="z", count=None, leaf: float = 0.5, num_threads: int = 1):
    """-> (cloud f32 [B,3,N], field f32 [B,N], count i32 [B])"""
    a, c = _frames_np(pc, count)
    B, _, N = a.shape
    axis, supplied = _field(field, (B, N), a)
    supplied = None if supplied is None else np.ascontiguousarray(supplied)
    keys = np.zeros((B, N), np.int64)
    _lib.check(_lib.lib().usip_sift_voxel_keys_f32_cpu(_p(a), _p(c), B, N, float(leaf), _p(keys)), "usip_sift_voxel_keys_f32_cpu")
    cloud, fld, cnt = np.zeros((B, 3, N), np.float32), np.zeros((B, N), np.float32), np.zeros((B,), np.int32)
    _lib.check(_lib.lib().usip_sift_voxel_average_f32_cpu(_p(a), _p(supplied), axis, _p(keys), B, N, _p(cloud), _p(fld), _p(cnt),
                                                          int(num_threads)), "usip_sift_voxel_average_f32_cpu")
    return cloud, fld, cnt


def sift_dog_cpu(cloud, field, count, sigma2, num_threads: int = 1):
    """-> dog f64 [B,S-1,N] from the S values sigma_s^2"""
    a, c = _frames_np(cloud, count)
    B, _, N = a.shape
    f = np.ascontiguousarray(field, dtype=np.float32)
    s2 = np.ascontiguousarray(sigma2, dtype=np.float64)
    if f.shape != (B, N) or s2.ndim != 1:
        raise ValueError("sift: expected field f32 [B,N] and sigma2 f64 [S]")
    dog = np.zeros((B, max(s2.shape[0] - 1, 1), N), np.float64)
    _lib.check(_lib.lib().usip_sift_dog_f32_cpu(_p(a), _p(f), _p(c), B, N, s2.shape[0], _p(s2), _p(dog), int(num_threads)),
               "usip_sift_dog_f32_cpu")
    return dog


def sift_scale_space_cpu(cloud, field, count, base: float, n_scales_per_octave: int = 8, num_threads: int = 1):
    _check_sift(base, 1, n_scales_per_octave, 0.0)
    return sift_dog_cpu(cloud, field, count, sift_sigma2(base, n_scales_per_octave), num_threads)


def sift_nearest_cpu(cloud, count, num_threads: int = 1):
    """-> idx i32 [B,N,25]"""
    a, c = _frames_np(cloud, count)
    B, _, N = a.shape
    idx = np.zeros((B, N, ops.SIFT_NEAREST), np.int32)
    _lib.check(_lib.lib().usip_sift_nearest_f32_cpu(_p(a), _p(c), B, N, _p(idx), int(num_threads)), "usip_sift_nearest_f32_cpu")
    return idx


def sift_extrema_cpu(dog, idx, count, min_contrast: float, num_threads: int = 1):
    """-> (mask u8 [B,N], scale_index i32 [B,N])"""
    d = np.ascontiguousarray(dog, dtype=np.float64)
    B, S1, N = d.shape
    i = np.ascontiguousarray(idx, dtype=np.int32)
    c = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
    if i.shape != (B, N, ops.SIFT_NEAREST):
        raise ValueError("sift: expected idx i32 [B,N,25]")
    mask, sidx = np.zeros((B, N), np.uint8), np.zeros((B, N), np.int32)
    _lib.check(_lib.lib().usip_sift_extrema_f32_cpu(_p(d), _p(i), _p(c), B, N, S1 + 1, float(min_contrast), _p(mask), _p(sidx),
                                                    int(num_threads)), "usip_sift_extrema_f32_cpu")
    return mask, sidx


def sift_keypoints_cpu(pc, count=None, min_scale: float = 0.5, n_octaves: int = 4, n_scales_per_octave: int = 8,
                       min_contrast: float = 0.1, field="z", want_octaves: bool = False, num_threads: int = 1):
    """-> (candidates f32 [B,3,O*N], mask u8 [B,O*N], scale f64 [B,O*N], octave_count i32 [B,O])[, octaves]"""
    _check_sift(min_scale, n_octaves, n_scales_per_octave, min_contrast)
    cloud, cnt = _frames_np(pc, count)
    fld = field
    clouds, masks, scales, counts, octaves = [], [], [], [], []
    for o in range(int(n_octaves)):
        base = float(min_scale) * 2.0 ** o
        cloud, fld, cnt = sift_octave_cpu(cloud, field if isinstance(field, str) else fld, cnt, base, num_threads)
        sigma2 = sift_sigma2(base, n_scales_per_octave)
        dog = sift_dog_cpu(cloud, fld, cnt, sigma2, num_threads)
        idx = sift_nearest_cpu(cloud, cnt, num_threads)
        mask, sidx = sift_extrema_cpu(dog, idx, cnt, min_contrast, num_threads)
        clouds.append(cloud)
        masks.append(mask)
        scales.append(np.where(mask != 0, np.sqrt(sigma2)[sidx], 0.0))
        counts.append(cnt)
        octaves.append((cloud, fld, cnt, dog, idx, mask, sidx))
    out = (np.concatenate(clouds, 2), np.concatenate(masks, 1), np.concatenate(scales, 1), np.stack(counts, 1))
    return out + (octaves,) if want_octaves else out


def select_candidates_cpu(pc, count, candidates, mask, num: int, ensure: bool = True, seed: int = 0, frame_ids=None,
                          want_index: bool = False):
    a, c = _frames_np(pc, count)
    cand = np.ascontiguousarray(candidates, dtype=np.float32)
    u = _draws(a.shape[0], cand.shape[2] + a.shape[2], seed, frame_ids)
    kp, cnt, order = _select_candidates(torch.from_numpy(a), None if c is None else torch.from_numpy(c), torch.from_numpy(cand),
                                        torch.from_numpy(np.ascontiguousarray(mask)), num, ensure, u)
    return (kp.numpy(), cnt.numpy(), order.numpy()) if want_index else (kp.numpy(), cnt.numpy())


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
