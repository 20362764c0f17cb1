"""Evaluation batches of indoor fragments built on the GPU, and fragments described from checkpoints.

The reference evaluates its indoor model with two CPU loaders (RedwoodLoader.__getitem__, evaluation/redwood_loader.py:73-127;
Match3DEvalLoader.__getitem__, data/match3d_eval_loader.py:78-103) that draw N rows of a fragment file, N/2 FPS candidates
among them and M farthest-point nodes in numpy, and the `tsf` branch of evaluation/save_keypoints.py:262-351 that runs the
detector, NMS / top-k and the descriptor on every batch.  Here the fragments live in HBM (FragmentScanBank), one call
enqueues a batch on the current stream with no host synchronisation (csrc/fragment_batch.hip), and FragmentDescriber runs
the two eval-mode networks on it:

    bank = FragmentScanBank.from_scene_dir(scene_dir, "cuda:0")
    builder = FragmentBatchBuilder(bank, FragmentBatchRecipe.match3d(opt), seed=0)
    describer = FragmentDescriber(detector, descriptor, builder, nms_radius=0.1, top=512)
    for ids in batches_of(range(bank.num_scans), 8):
        out = describer.describe(ids)
        evaluator.add_described(ids, out["kp"], out["desc"], out["count"], [bank.xyz(i) for i in ids])

Randomness is Philox4x64-10 keyed by the seed, counter (element, stream, FRAGMENT ID, step), stream tags 49-51: a fragment
gets the same points and nodes whatever batch it rides in, and no draw is shared with usip_amd.pairs (1-8),
usip_amd.desc_pairs (17-26) or usip_amd.indoor_pairs (33-40) under one seed.

Two stated deviations from the reference:
  1. A fragment with fewer than N rows takes RedwoodLoader's fix_idx layout (whole copies of 0..n-1, then a draw of the
     remainder) under both presets; Match3DEvalLoader's np.random.choice would raise there.
  2. save_keypoints.py:348-349 shrinks desired_keypoint_num for every LATER frame once one frame has fewer NMS survivors;
     here every fragment keeps up to `top` of its own, whatever came before it.
The script's noise_sigma robustness experiment is not here.
"""
import os
import re
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import inference, ops
from .evaluation import select_keypoints_device
from .pairs import ScanBank, _CloudBuilder, host_twin

KEYS = ops.FRAGMENT_BATCH_KEYS
_FILE = re.compile(r"(?:cloud_bin_)?(\d+)\.npy")


def scene_files(scene_dir: str):
    """The fragment files of a scene directory, cloud_bin_<i>.npy (3DMatch) or <i>.npy (Redwood), as (ids in numeric order,
    paths)."""
    found = {}
    for name in os.listdir(scene_dir):
        m = _FILE.fullmatch(name)
        if m:
            if int(m.group(1)) in found:
                raise ValueError("FragmentScanBank: %s holds fragment %d under two names" % (scene_dir, int(m.group(1))))
            found[int(m.group(1))] = os.path.join(scene_dir, name)
    if not found:
        raise ValueError("FragmentScanBank: no cloud_bin_<i>.npy or <i>.npy in %s" % scene_dir)
    ids = sorted(found)
    return ids, [found[i] for i in ids]


def load_scene_dir(scene_dir: str):
    """(the files' own numbers in numeric order, their arrays): what from_scene_dir uploads and build_cpu takes."""
    ids, paths = scene_files(scene_dir)
    return ids, [np.load(p) for p in paths]


def with_normals(xyz: torch.Tensor, k: int = 9) -> torch.Tensor:
    """xyz f32 [n,3] on the device -> f32 [n,7] x y z nx ny nz curvature: prepare.ScanPreparer.normals with k neighbours,
    the viewpoint at the fragment frame's origin and no grid average -- what the reference's findPointNormals.m did for
    its files."""
    from .prepare import ScanPreparer
    prep = ScanPreparer(xyz.device, k=k, viewpoint=(0.0, 0.0, 0.0))
    xyzi = torch.cat((xyz, xyz.new_zeros(xyz.shape[0], 1)), 1)
    nrm, _ = prep.normals(xyzi)
    return torch.cat((xyz, nrm.to(torch.float32)), 1).contiguous()


class FragmentScanBank(ScanBank):
    """A ScanBank of a scene's fragments, rows x y z nx ny nz curvature ...; fragment_ids are the files' own numbers, the
    bank's ids are positions in that order.  xyz(id) is the fragment's device cloud [rows, 3], what FragmentEvaluator
    stores beside the keypoints: a file is read once."""

    def __init__(self, scans: Sequence, device, row_len: int = 7, reserve: float = 0.1, fragment_ids=None):
        super().__init__(list(scans), device, row_len=row_len, radius_threshold=100.0, reserve=reserve)
        self.fragment_ids = list(range(self.num_scans)) if fragment_ids is None else [int(i) for i in fragment_ids]

    @classmethod
    def from_device_rows(cls, scans: Sequence[torch.Tensor], device=None, row_len: int = 7, fragment_ids=None):
        self = super().from_device_rows(list(scans), device=device, row_len=row_len, radius_threshold=100.0)
        self.fragment_ids = list(range(self.num_scans)) if fragment_ids is None else [int(i) for i in fragment_ids]
        return self

    @classmethod
    def from_arrays(cls, arrays: Sequence, device, normals_k: int = 9, fragment_ids=None) -> "FragmentScanBank":
        """numpy [rows, C] arrays of one C: C >= 7 are taken as they are; C == 3 (xyz only) get normals and curvature on
        the device (with_normals)."""
        arrays = [np.asarray(a) for a in arrays]
        if not arrays or any(a.ndim != 2 or a.shape[1] != arrays[0].shape[1] for a in arrays):
            raise ValueError("FragmentScanBank: fragments are [rows, C] arrays of one C")
        C = arrays[0].shape[1]
        if C == 3:
            dev = torch.device(device)
            rows = []
            for i, a in enumerate(arrays):
                if a.shape[0] < normals_k:
                    raise ValueError("FragmentScanBank: fragment %d has %d rows, normals need %d" % (i, a.shape[0], normals_k))
                rows.append(with_normals(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev), normals_k))
            return cls.from_device_rows(rows, device=dev, row_len=7, fragment_ids=fragment_ids)
        if C < 7:
            raise ValueError("FragmentScanBank: rows are x y z, or x y z nx ny nz curvature ...; got %d columns" % C)
        return cls(arrays, device, row_len=C, fragment_ids=fragment_ids)

    @classmethod
    def from_scene_dir(cls, scene_dir: str, device, normals_k: int = 9) -> "FragmentScanBank":
        ids, arrays = load_scene_dir(scene_dir)
        return cls.from_arrays(arrays, device, normals_k=normals_k, fragment_ids=ids)

    def xyz(self, i: int) -> torch.Tensor:
        return self.rows[int(self.offsets_host[i]):int(self.offsets_host[i + 1]), :3].contiguous()


@dataclass
class FragmentBatchRecipe:
    """What one evaluation fragment is made of: N points, n_sub FPS candidates among them, M nodes, Cs sn channels."""
    N: int = 10240
    M: int = 512
    Cs: int = 4
    n_sub: int = 5120

    @classmethod
    def match3d(cls, opt, downsample_rate: float = 1) -> "FragmentBatchRecipe":
        """match3d/options_detector.py and scenenn/options_detector.py: input_pc_num / downsample_rate points, half of
        them FPS candidates, node_num nodes."""
        g = lambda k, d: getattr(opt, k, d)   # noqa: E731
        N = int(int(g("input_pc_num", 10240)) / downsample_rate)
        return cls(N=N, M=int(g("node_num", 512)), Cs=int(g("surface_normal_len", 4)), n_sub=int(N / 2))

    def c_struct(self, row_len: int) -> ops.PairsRecipeC:
        r = ops.PairsRecipeC()
        r.N, r.M, r.Cs, r.n_sub, r.row_len = self.N, self.M, self.Cs, self.n_sub, int(row_len)
        return r


class FragmentBatchBuilder(_CloudBuilder):
    """Any number of fragments per call, written as the eval-mode detector and descriptor consume them: pc f32 [B,3,N], sn
    f32 [B,Cs,N], node f32 [B,3,M].  An odd B is built beside one repeated cloud (the cloud stage works in two halves) and
    the first B rows are returned.

    build(ids, step=0, out=None, with_indices=False): Philox draws keyed by the fragment's id.  `out`: buffers of
        ops.fragment_batch_shapes(c, B) to write into.
    apply(ids, draws): the recorded draws of the reference (tests): rows [B,N], cand [B,n_sub], first [B]."""

    spec = ops.FRAGMENT_BATCH
    _modes = ("eval",)

    def __init__(self, bank: FragmentScanBank, recipe: FragmentBatchRecipe, device=None, seed: int = 0):
        self._wsb = {}
        super().__init__(bank, recipe, 0, device, seed, 0, "eval")

    def _c_struct(self):
        return self.recipe.c_struct(self.bank.row_len)

    def _check(self):
        if 3 + self.recipe.Cs > self.bank.row_len:
            raise ValueError("FragmentBatchBuilder: fragments of %d columns hold no %d sn channels after x y z"
                             % (self.bank.row_len, self.recipe.Cs))
        ops.fragment_batch_workspace_bytes(self.c, 1)                # an invalid recipe is refused here

    def _workspace(self, B: int, which: int = 0) -> torch.Tensor:
        """One workspace per number of clouds met."""
        B2 = ops.fragment_batch_clouds(B)
        if B2 not in self._wsb:
            self._wsb[B2] = torch.empty(ops.fragment_batch_workspace_bytes(self.c, B2), dtype=torch.uint8, device=self.device)
        return self._wsb[B2]

    def _of_call(self, tensors: dict, B: int) -> dict:
        return {k: t[:B] for k, t in tensors.items()}

    def _counter(self, step: int) -> tuple:
        return (self.seed, int(step))

    def build(self, ids, step: int = 0, out: Optional[Dict[str, torch.Tensor]] = None, with_indices: bool = False):
        return super().build(ids, step, out, with_indices)

    def prefetch(self, schedule, outs=None):
        raise NotImplementedError("FragmentBatchBuilder: evaluation batches are built in line")

    def build_cpu(self, ids, fragments: Sequence[np.ndarray], step: int = 0, draws=None, num_threads: int = 1):
        """The host twin on the same recipe and seed; fragments: the bank's numpy rows."""
        return build_cpu(self.recipe, fragments, ids, seed=self.seed, step=step, draws=draws, num_threads=num_threads)


def build_cpu(recipe: FragmentBatchRecipe, fragments: Sequence[np.ndarray], ids, seed: int = 0, step: int = 0,
              draws: Optional[Dict[str, np.ndarray]] = None, num_threads: int = 1):
    """The host twin (usip_fragment_batch_build_f32_cpu) on numpy fragments [rows, row_len]: Philox draws, or `draws` (rows
    [B,N], cand [B,n_sub], first [B]).  Returns (batch of pc / sn / node, rows [B,N], node_slots [B,M])."""
    h = np.asarray(ids, dtype=np.int64).reshape(-1)
    if h.size < 1 or h.min() < 0 or h.max() >= len(fragments):
        raise ValueError("build_cpu: fragment id out of range [0, %d)" % len(fragments))
    out, rows, nodes = host_twin(ops.FRAGMENT_BATCH, recipe.c_struct, fragments, "fragment", h, None, counter=(seed, step),
                                 draws=draws, num_threads=num_threads)
    return {k: v[:h.size] for k, v in out.items()}, rows[:h.size], nodes[:h.size]


class FragmentDescriber:
    """The `tsf` branch of evaluation/save_keypoints.py:262-351 on built batches: the eval-mode detector, sigma-ordered NMS
    and top-k (evaluation.select_keypoints_device, padded with the fragment's first pick), then the eval-mode descriptor
    on the same N points under inference.describe_keypoints' fixed permutation, which lives on the device, cached per N.
    Nothing synchronises with the host.

    describe(ids, step=0) -> dict(kp f32 [B,3,top], desc f32 [B,D,top], count i32 [B], sigmas f32 [B,M], keypoints f32
        [B,3,M] (the detector's, before the selection), pc, sn, node).
    keypoints(ids, step=0) -> the same without desc: the detector only.
    describe_keypoints(ids, kp, count, step=0): the learned descriptor on another detector's keypoints kp [B,3,M']."""

    def __init__(self, detector, descriptor, builder: FragmentBatchBuilder, nms_radius: float = 0.1, top: int = 512,
                 perm_seed: int = 0):
        self.detector, self.descriptor, self.builder = detector, descriptor, builder
        self.nms_radius, self.top, self.perm_seed = float(nms_radius), int(top), int(perm_seed)
        self._perm = {}

    def perm(self, N: int) -> torch.Tensor:
        if N not in self._perm:
            p = np.random.default_rng(self.perm_seed).permutation(int(N))
            self._perm[N] = torch.from_numpy(p).pin_memory().to(self.builder.device, non_blocking=True)
        return self._perm[N]

    def _describe(self, pc, sn, kp):
        if self.descriptor is None:
            raise ValueError("FragmentDescriber: no descriptor")
        self.descriptor.eval()
        with torch.no_grad():
            desc, _ = self.descriptor(pc, sn, kp.contiguous(), False, None, perm=self.perm(pc.shape[2]))
        return desc

    def keypoints(self, ids, step: int = 0) -> Dict[str, torch.Tensor]:
        if self.detector is None:
            raise ValueError("FragmentDescriber: no detector")
        batch = self.builder.build(ids, step)
        keypoints, sigmas = inference.run_model(self.detector, batch["pc"], batch["sn"], batch["node"])
        kp, count = select_keypoints_device(keypoints, sigmas, self.nms_radius, self.top)
        return dict(batch, kp=kp, count=count, sigmas=sigmas, keypoints=keypoints)

    def describe(self, ids, step: int = 0) -> Dict[str, torch.Tensor]:
        out = self.keypoints(ids, step)
        out["desc"] = self._describe(out["pc"], out["sn"], out["kp"])
        return out

    def describe_keypoints(self, ids, kp: torch.Tensor, count: torch.Tensor, step: int = 0) -> Dict[str, torch.Tensor]:
        batch = self.builder.build(ids, step)
        B = batch["pc"].shape[0]
        if kp.dim() != 3 or kp.shape[0] != B or kp.shape[1] != 3 or kp.shape[2] < 1:
            raise ValueError("describe_keypoints: expected kp [%d,3,M'], got %s" % (B, tuple(kp.shape)))
        kp = kp.to(self.builder.device, torch.float32).contiguous()
        count = torch.clamp(count.to(self.builder.device, torch.int32).reshape(B), max=kp.shape[2])
        return dict(batch, kp=kp, count=count, desc=self._describe(batch["pc"], batch["sn"], kp))


def write_keypoints_dir(directory: str, fragment_ids, kp: torch.Tensor, count: torch.Tensor):
    """<directory>/<id>.bin per fragment: its first count keypoints as float32 [count, 3] rows, the file eval_rep.m reads
    (save_keypoints.py:392-393).  One host read."""
    os.makedirs(directory, exist_ok=True)
    kp_h, count_h = kp.detach().cpu().numpy(), count.detach().cpu().numpy()
    for b, i in enumerate(fragment_ids):
        inference.write_keypoints_bin(os.path.join(directory, "%d.bin" % int(i)),
                                      np.ascontiguousarray(kp_h[b][:, :int(count_h[b])].T))
