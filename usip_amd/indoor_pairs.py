"""Indoor descriptor training batches built on the GPU from SceneNN frame pairs.

The reference builds every (anchor, positive) pair on the CPU in DataLoader workers (SceneNNDescriptorLoader.__getitem__,
data/scenenn_descriptor_loader.py:230-289): two frames of a recorded pair, the anchor moved into the positive's frame by the
pair's 4x4 ICP matrix in float64, two farthest-point samplings in numpy, ONE augmentation for both clouds, then
transform_pc_pytorch on the positive.  Here the frames, the pair list and the matrices live in HBM (IndoorPairBank) and one
call enqueues the whole batch on the current stream, with no host synchronisation (csrc/indoor_pairs.hip):

    train = IndoorPairBank.from_root(root, "train", "cuda:0") + IndoorPairBank.from_root(root, "val", "cuda:0")
    builder = IndoorPairBuilder(train, IndoorPairRecipe.scenenn(opt), pairs=2, seed=0, mode="bank")
    trainer = IndoorDescriptorTrainer(builder, "ball", detector_state, opt)
    for step, ids in enumerate(epoch_batches(train.num_samples, 2, seed=0, epoch=0)):
        trainer.train_step(builder.build(ids, step), epoch=0)

Randomness is Philox4x64-10 keyed by the seed, counter (element, stream, rank * P + p, step), stream tags 33-40: no draw is
shared with usip_amd.pairs (1-8) or usip_amd.desc_pairs (17-26) under one seed.

The one stated deviation a user may choose: the reference adds the ICP TRANSLATION to the anchor's normals (it sends
sn[:, 0:3] through the same homogeneous product as the points).  IndoorPairRecipe.icp_moves_normals = 1 (the default)
reproduces that; 0 rotates the normals only.
"""
import os
import pickle
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import ops
from .desc_pairs import _FrozenDetectorTrainer
from .pairs import ScanBank, _CloudBuilder, _empty_batch, bank_arrays, host_twin
from .pairs import epoch_batches, epoch_order          # noqa: F401  (re-exported)

KEYS = ops.INDOOR_PAIRS_KEYS
MODES = {"train": 0, "val": 1, "test": 2, "bank": 3}


@dataclass
class IndoorPairRecipe:
    """What one indoor pair is made of (usip_indoor_pairs_recipe, include/usip_hip.h), bar the mode, which the builder
    sets, and row_len, which is the bank's.  The reference draws jitter and never adds it: there is no sigma here."""
    N: int = 5000
    M: int = 512
    Cs: int = 4
    n_sub: int = 2500
    rot_horizontal: int = 1
    rot_3d: int = 0
    rot_perturbation: int = 1
    translation_perturbation: int = 0
    aug_scale_lo: float = 0.9
    aug_scale_hi: float = 1.1
    shift_range: float = 1.0
    pert_sigma: float = 0.12
    pert_clip: float = 0.36
    dst_scale_thre: float = 0.2              # transform_pc_pytorch's default, which the loader does not override
    dst_shift_thre: float = 0.5
    icp_moves_normals: int = 1

    @classmethod
    def scenenn(cls, opt) -> "IndoorPairRecipe":
        """SceneNNDescriptorLoader (scenenn/options_descriptor.py): N/2 FPS candidates, node_num nodes, augment scale
        U(0.9, 1.1), perturbation 0.12 clipped at 0.36, transform_pc_pytorch(rot_type, shift_thre=0.5)."""
        g = lambda k, d: getattr(opt, k, d)   # noqa: E731
        N = int(g("input_pc_num", 5000))
        return cls(N=N, M=int(g("node_num", 512)), Cs=int(g("surface_normal_len", 4)), n_sub=int(N / 2),
                   rot_horizontal=int(bool(g("rot_horizontal", True))), rot_3d=int(bool(g("rot_3d", False))),
                   rot_perturbation=int(bool(g("rot_perturbation", True))),
                   translation_perturbation=int(bool(g("translation_perturbation", False))))

    def c_struct(self, mode: str, row_len: int) -> ops.IndoorPairsRecipeC:
        if mode not in MODES:
            raise ValueError("IndoorPairRecipe: mode is one of %s" % ", ".join(MODES))
        r = ops.IndoorPairsRecipeC()
        for k in ("N", "M", "Cs", "n_sub", "rot_horizontal", "rot_3d", "rot_perturbation", "translation_perturbation",
                  "aug_scale_lo", "aug_scale_hi", "shift_range", "pert_sigma", "pert_clip", "dst_scale_thre",
                  "dst_shift_thre"):
            setattr(r.cloud, k, getattr(self, k))
        r.cloud.row_len = int(row_len)
        r.cloud.dst_rot_type = 3 if self.rot_3d else (2 if self.rot_horizontal else 0)
        r.cloud.dst_rot_perturbation = int(bool(self.rot_perturbation))
        r.icp_moves_normals, r.mode = int(self.icp_moves_normals), MODES[mode]
        return r


def check_samples(pairs, icp, num_frames: int):
    """pairs -> i32 [S, 2], icp [S, 4, 4] -> f64 [S, 12] (rows 0..2), refusing what the kernels would only clamp."""
    pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int64)
    icp = np.asarray(icp, dtype=np.float64)
    S = pairs.shape[0]
    if S < 1:
        raise ValueError("IndoorPairBank: no samples")
    if icp.shape != (S, 4, 4):
        raise ValueError("IndoorPairBank: icp must be [%d, 4, 4] for %d pairs, got %s" % (S, S, icp.shape))
    if pairs.min() < 0 or pairs.max() >= num_frames:
        raise ValueError("IndoorPairBank: a pair names frame %d, the bank has frames 0..%d"
                         % (int(pairs.max() if pairs.max() >= num_frames else pairs.min()), num_frames - 1))
    bad = np.flatnonzero((icp[:, 3, :] != np.array([0.0, 0.0, 0.0, 1.0])).any(axis=1))
    if bad.size:
        raise ValueError("IndoorPairBank: the last row of sample %d's ICP matrix is %s, not (0, 0, 0, 1)"
                         % (int(bad[0]), icp[bad[0], 3].tolist()))
    return pairs.astype(np.int32), np.ascontiguousarray(icp[:, :3, :].reshape(S, 12))


def _thin(mode: str, pairs, icp):
    """SceneNNDescriptorLoader.__init__ :93-96: mode 'test' keeps samples 0, 3, 6, ..."""
    pairs, icp = np.asarray(pairs), np.asarray(icp)
    return (pairs[::3], icp[::3]) if mode == "test" else (pairs, icp)


class IndoorPairBank(ScanBank):
    """A ScanBank of frames plus the samples that pair them: pairs i32 [S, 2] (anchor frame, positive frame), icp f64
    [S, 12] (rows 0..2 of each 4x4 matrix) and every sample's mode, on the device.  `a + b` concatenates two banks
    (train + val, as the reference's concatenated dataset), each sample keeping its mode."""

    def __init__(self, frames: Sequence, pairs, icp, device, mode: str = "train", row_len: int = 7, reserve: float = 0.1):
        super().__init__(list(frames), device, row_len=row_len, radius_threshold=100.0, reserve=reserve)
        self._set_samples(pairs, icp, mode)

    def _set_samples(self, pairs, icp, mode):
        if isinstance(mode, str):
            if mode not in ("train", "val", "test"):
                raise ValueError("IndoorPairBank: mode is 'train', 'val' or 'test'")
            mode = np.full(len(np.asarray(pairs).reshape(-1, 2)), MODES[mode], dtype=np.int32)
        self.pairs_host, self.icp_host = check_samples(pairs, icp, self.num_scans)
        self.mode_host = np.ascontiguousarray(mode, dtype=np.int32)
        self.num_samples = self.pairs_host.shape[0]
        self.pairs = torch.from_numpy(self.pairs_host).to(self.device)
        self.icp = torch.from_numpy(self.icp_host).to(self.device)
        self.sample_mode = torch.from_numpy(self.mode_host).to(self.device)

    @classmethod
    def from_arrays(cls, frames: Sequence, pairs, icp, device, mode: str = "train", row_len: int = 7, **kw):
        return cls(frames, pairs, icp, device, mode=mode, row_len=row_len, **kw)

    @classmethod
    def from_root(cls, root: str, mode: str, device, row_len: Optional[int] = None, **kw) -> "IndoorPairBank":
        """<root>/info_<mode>.pkl (pairs_np [S, 2], icp_np [S, 4, 4]) and the frames it names, <root>/frames_<mode>/<i>.npy;
        mode 'test' keeps every third sample.  Only the frames some kept sample names are read; they are renumbered."""
        paths, pairs, icp, used = root_layout(root, mode)
        if row_len is None:
            row_len = int(np.load(paths[0], mmap_mode="r").shape[1])
        self = cls(paths, pairs, icp, device, mode=mode, row_len=row_len, **kw)
        self.frame_ids = used
        return self

    @classmethod
    def from_device_rows(cls, frames: Sequence[torch.Tensor], pairs, icp, device=None, mode: str = "train",
                         row_len: int = 7) -> "IndoorPairBank":
        """The bank of float32 [rows, row_len] tensors already in device memory."""
        self = super().from_device_rows(list(frames), device=device, row_len=row_len, radius_threshold=100.0)
        self._set_samples(pairs, icp, mode)
        return self

    def __add__(self, other: "IndoorPairBank") -> "IndoorPairBank":
        if not isinstance(other, IndoorPairBank) or other.row_len != self.row_len or other.device != self.device:
            raise ValueError("IndoorPairBank: only two banks of one row length on one device concatenate")
        new = IndoorPairBank.__new__(IndoorPairBank)
        new.device, new.row_len = self.device, self.row_len
        new.lengths = np.concatenate([self.lengths, other.lengths])
        new.offsets_host = np.concatenate([[0], np.cumsum(new.lengths)]).astype(np.int64)
        new.rows = torch.cat([self.rows, other.rows])
        new.offsets = torch.from_numpy(new.offsets_host).to(new.device)
        new.num_scans, new.min_rows = self.num_scans + other.num_scans, min(self.min_rows, other.min_rows)
        new._set_samples(*concat_samples(self.num_scans, (self.pairs_host, self.icp_host, self.mode_host),
                                         (other.pairs_host, other.icp_host, other.mode_host)))
        return new

    def c_dict(self) -> dict:
        """What ops.indoor_pairs_build takes as `bank`."""
        return dict(rows=self.rows, offsets=self.offsets, pairs=self.pairs, icp=self.icp, sample_mode=self.sample_mode,
                    pairs_host=self.pairs_host, min_rows=self.min_rows)


def root_layout(root: str, mode: str):
    """SceneNNDescriptorLoader.__init__ (:72-96) on <root>: (frame paths, pairs [S, 2] renumbered onto them, icp [S, 4, 4],
    the frames' own numbers).  Mode 'test' keeps samples 0, 3, 6, ...; only frames a kept sample names are listed."""
    with open(os.path.join(root, "info_%s.pkl" % mode), "rb") as f:
        info = pickle.load(f)
    pairs, icp = _thin(mode, np.asarray(info["pairs_np"]).reshape(-1, 2), np.asarray(info["icp_np"], dtype=np.float64))
    used, inverse = np.unique(pairs.reshape(-1), return_inverse=True)
    paths = [os.path.join(root, "frames_" + mode, "%d.npy" % i) for i in used]
    return paths, inverse.reshape(-1, 2), icp, used


def load_root(root: str, mode: str):
    """root_layout with the frames read: (frames, pairs, icp), what build_cpu takes."""
    paths, pairs, icp, _ = root_layout(root, mode)
    return [np.load(p) for p in paths], pairs, icp


def concat_samples(frames_a: int, a, b):
    """(pairs, icp rows [S, 12] or matrices [S, 4, 4], modes) of two banks -> those of `a + b`, as [S, 2], [S, 4, 4], [S]:
    b's frame ids move up by a's frames_a frames, every sample keeps its mode."""
    def full(icp):
        icp = np.asarray(icp, dtype=np.float64)
        if icp.shape[1:] == (4, 4):
            return icp
        out = np.zeros((icp.shape[0], 4, 4))
        out[:, 3, 3] = 1.0
        out[:, :3, :] = icp.reshape(-1, 3, 4)
        return out
    return (np.concatenate([np.asarray(a[0]), np.asarray(b[0]) + int(frames_a)]), np.concatenate([full(a[1]), full(b[1])]),
            np.concatenate([np.asarray(a[2], dtype=np.int32), np.asarray(b[2], dtype=np.int32)]))


def synthetic_scenenn(root: str, frames: int = 6, rows: int = 6000, short_rows: Optional[int] = None, seed: int = 0,
                      modes: Sequence[str] = ("train", "val", "test"), extent: float = 3.0) -> Dict[str, int]:
    """Write a small dataset in the reference's on-disk layout under `root`: info_<mode>.pkl with pairs_np [S, 2] and
    icp_np [S, 4, 4], frames_<mode>/<i>.npy as float32 [rows, 7] (x y z nx ny nz curvature).  Every mode has one slab
    scene (synth.make_cloud) seen from `frames` known poses a few tenths of a radian and about a metre apart; a sample
    pairs neighbouring frames in both orders, and icp is the true relative pose (anchor frame -> positive frame), so
    the moved anchor lies on the positive.  short_rows: the last frame has that many rows (the fix_idx layout).
    Returns {mode: number of samples}."""
    from . import synth
    out = {}
    for mi, mode in enumerate(modes):
        rng = np.random.default_rng([int(seed), mi])
        n_scene = 3 * rows
        world = synth.make_cloud(rng, n_scene, "slab:%g" % extent).T.astype(np.float64)
        world[:, 1] *= 0.05                                                   # a thin slab: metres, as an indoor wall
        extra = synth.make_normals(rng, n_scene, 4).T.astype(np.float64)      # nx ny nz curvature
        poses = []
        os.makedirs(os.path.join(root, "frames_" + mode), exist_ok=True)
        for i in range(frames):
            ax, ay, az = rng.normal(0, 0.05), 0.15 * i + rng.normal(0, 0.02), rng.normal(0, 0.05)
            cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
            R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
                 @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, [0.4 * i + rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.2)]
            poses.append(T)
            n = int(short_rows) if (short_rows and i == frames - 1) else rows
            pick = rng.choice(n_scene, n, replace=False)
            local = (world[pick] - T[:3, 3]) @ R                              # R' (p - t) as row vectors
            frame = np.concatenate([local, extra[pick, :3] @ R, extra[pick, 3:]], 1).astype(np.float32)
            np.save(os.path.join(root, "frames_" + mode, "%d.npy" % i), frame)
        pairs, icp = [], []
        for i in range(frames - 1):
            for a, b in ((i, i + 1), (i + 1, i)):
                pairs.append((a, b))
                icp.append(np.linalg.inv(poses[b]) @ poses[a])
        icp = np.stack(icp)
        icp[:, 3, :] = [0.0, 0.0, 0.0, 1.0]
        with open(os.path.join(root, "info_%s.pkl" % mode), "wb") as f:
            pickle.dump(dict(pairs_np=np.asarray(pairs, dtype=np.int64), icp_np=icp), f)
        out[mode] = len(pairs)
    return out


def empty_batch(c: ops.IndoorPairsRecipeC, pairs: int, device) -> Dict[str, torch.Tensor]:
    return _empty_batch(ops.INDOOR_PAIRS, c, pairs, device)


class IndoorPairBuilder(_CloudBuilder):
    """P (anchor, positive) pairs per call, written as IndoorDescriptorStep.step consumes them.

    mode: 'train', 'val', 'test' for every sample of a call, or 'bank': each sample's own (a train + val bank).
    build(sample_ids, step, out=None): Philox draws.  `out` may hold any of KEYS (e.g. IndoorDescriptorStep.static_batch's
        buffers), which are then written in place; the rest is allocated.
    apply(sample_ids, draws, out=None): the recorded draws of the reference (tests).
    prefetch(schedule): double-buffered, batch k+1 built on a side stream while the consumer runs batch k."""

    spec = ops.INDOOR_PAIRS
    _modes = tuple(MODES)

    def _c_struct(self):
        return self.recipe.c_struct(self.mode, self.bank.row_len)

    def _num_ids(self) -> int:
        return self.bank.num_samples

    def _check(self):
        if 3 + self.recipe.Cs > self.bank.row_len:
            raise ValueError("IndoorPairBuilder: frames of %d columns hold no %d sn channels after x y z"
                             % (self.bank.row_len, self.recipe.Cs))
        if self.recipe.Cs < 3:
            raise ValueError("IndoorPairBuilder: the ICP move acts on sn[0:3]: surface_normal_len >= 3")


def build_cpu(recipe: IndoorPairRecipe, frames: Sequence[np.ndarray], pairs, icp, sample_ids, num_pairs: int,
              seed: int = 0, step: int = 0, rank: int = 0, mode: str = "train", sample_mode=None,
              draws: Optional[Dict[str, np.ndarray]] = None, num_threads: int = 1):
    """The host twin (usip_indoor_pairs_build_f32_cpu) on numpy frames, pairs [S, 2] and icp [S, 4, 4]: Philox draws, or
    `draws` (f-5's layouts).  mode 'bank' reads sample_mode [S] (0 train, 1 val, 2 test).  Returns (batch, rows [2,P,N],
    node_slots [2,P,M]).  The same refusals as the bank's."""
    frames = bank_arrays(frames, "frame")
    pairs_h, icp_h = check_samples(pairs, icp, len(frames))
    modes = None if sample_mode is None else np.ascontiguousarray(sample_mode, dtype=np.int32).reshape(-1)
    if modes is not None and modes.size != pairs_h.shape[0]:
        raise ValueError("build_cpu: %d sample modes for %d samples" % (modes.size, pairs_h.shape[0]))
    return host_twin(ops.INDOOR_PAIRS, lambda row_len: recipe.c_struct(mode, row_len), frames, "frame", sample_ids,
                     num_pairs, bank=dict(pairs=pairs_h, icp=icp_h, sample_mode=modes, pairs_host=pairs_h),
                     counter=(seed, step, rank * int(num_pairs)), draws=draws, num_threads=num_threads)


class IndoorDescriptorTrainer(_FrozenDetectorTrainer):
    """scenenn/train_descriptor.py:99-141 and :157-226 on one device: a frozen detector gives the keypoints and sigmas of
    cat(anchor, positive) of every built batch, IndoorDescriptorStep trains on them, a pass over test-mode batches gates
    the checkpoint.  Everything of train_step is enqueued on the current stream; nothing is read back.  The reference's
    is_use_random_keypoint branch is not here."""

    def _make_step(self, opt, with_optimizer, graph, seed):
        from .step import IndoorDescriptorStep
        return IndoorDescriptorStep(opt, self.device, with_optimizer=with_optimizer, graph=graph, seed=seed)

    def descriptor_batch(self, batch: Dict[str, torch.Tensor], out: Optional[Dict[str, torch.Tensor]] = None):
        """The builder's batch -> what IndoorDescriptorStep consumes; with `out` (its static_batch) the keypoints, sigmas
        and permutation are written into it."""
        P, kp, sg, perm = self._keypoints(batch)
        d = dict(anc_kp=kp[:P].contiguous(), pos_kp=kp[P:].contiguous(), anc_sigmas=sg[:P].contiguous(), perm=perm)
        if out is not None:
            for k in d:
                out[k].copy_(d[k])
                d[k] = out[k]
        d.update({k: batch[k] for k in ("anc_pc", "pos_pc", "anc_sn", "pos_sn", "anc_R_pos", "anc_scale_pos",
                                        "anc_shift_pos")})
        return d

    def train_step(self, batch: Dict[str, torch.Tensor], epoch: Optional[int] = None, group=None, out=None):
        loss = self.st.step(self.descriptor_batch(batch, out), epoch=epoch, group=group)
        self.last_loss, self.last_active = loss, self.st.last["active_percentage"]
        return loss

    def test_pass(self, test_builder: IndoorPairBuilder, schedule: Iterable):
        """:157-226: IndoorDescriptorStep.test_model on test-mode batches, loss and active share averaged with the batch size
        as weight.  Returns (loss, active share) as floats -- the one read-back, once per pass."""
        loss_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        active_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        count = 0
        was_training = self.st.descriptor.training
        try:
            for ids, step in schedule:
                batch = test_builder.build(ids, step)
                B = batch["anc_pc"].shape[0]
                loss_sum += self.st.test_model(self.descriptor_batch(batch)).detach() * B
                active_sum += self.st.last["active_percentage"].detach() * B
                count += B
        finally:
            self.st.descriptor.train(was_training)
            self.st.triplet_criteria.train(was_training)
        if count == 0:
            raise ValueError("IndoorDescriptorTrainer.test_pass: an empty schedule")
        both = torch.stack((loss_sum, active_sum)).cpu()
        return float(both[0]) / count, float(both[1]) / count

    def _save_due(self, test_loss: float, epoch: int) -> bool:
        """:229: best so far from min_save_epoch on (the reference: epoch > 7.5, i.e. 8), or every tenth epoch."""
        return super()._save_due(test_loss, epoch) or (epoch > 1 and epoch % 10 == 0)
