"""Descriptor training batches built on the GPU from posed, device-resident scans.

The reference builds every (anchor, positive) pair on the CPU in DataLoader workers (KittiDescriptorLoader.__getitem__,
data/kitti_descriptor_loader.py:102-347) and mines the negatives on the host with an O(B^2) loop and a 4x4 inverse per
pair of anchors (mine_negative_sample, :278-317; kitti/train_descriptor.py:90-132).  Here the scans and their poses live
in HBM (PosedScanBank) and one call enqueues the whole batch -- the positive scan chosen by the reference's narrowing
search, subsampling, FPS nodes, each cloud's own augmentation, the negatives mined from the poses -- on the current
stream, with no host synchronisation (csrc/desc_pairs.hip):

    bank = PosedScanBank.from_sequences({0: (scans0, poses0), 1: (scans1, poses1)}, "cuda:0", min_points=opt.input_pc_num)
    builder = DescriptorPairBuilder(bank, DescriptorPairRecipe.kitti(opt), pairs=8, seed=0, rank=rank)
    trainer = DescriptorTrainer(builder, "ball", detector_state, opt)
    for step, ids in enumerate(epoch_batches(bank.num_scans, 8, seed=0, epoch=0, rank=rank, world=world)):
        trainer.train_step(builder.build(ids, step))

Randomness is Philox4x64-10 keyed by the seed, with counter (element, stream, rank * P + p, step) and stream tags of its
own (no draw is shared with usip_amd.pairs): a pair's clouds and its positive do not depend on the world size.
"""
import os
from dataclasses import dataclass
from typing import Dict, Iterable, Mapping, Optional, Sequence

import numpy as np
import torch

from . import ops
from .pairs import ScanBank, _CloudBuilder, _empty_batch, epoch_batches, epoch_order, host_twin   # noqa: F401  (re-exported)

KEYS = ops.DESC_PAIRS_KEYS


@dataclass
class DescriptorPairRecipe:
    """What one descriptor pair is made of (usip_desc_pairs_recipe, include/usip_hip.h), bar `train`, which the
    builder's mode sets.  The presets build it from the reference's option names; another data set (Oxford, SceneNN)
    is another preset over the same fields."""
    N: int = 16384
    M: int = 256
    Cs: int = 4
    n_sub: int = 4096
    row_len: int = 8
    rot_horizontal: int = 1
    rot_3d: int = 0
    rot_perturbation: int = 0
    translation_perturbation: int = 0
    aug_scale_lo: float = 0.9
    aug_scale_hi: float = 1.1
    shift_range: float = 1.0
    pc_sigma: float = 0.04
    pc_clip: float = 0.12
    sn_sigma: float = 0.01
    sn_clip: float = 0.05
    node_sigma: float = 0.04
    node_clip: float = 0.12
    pert_sigma: float = 0.06
    pert_clip: float = 0.18
    positive_radius: float = 5.0
    negative_radius: float = 50.0
    mine: int = 1

    @classmethod
    def kitti(cls, opt) -> "DescriptorPairRecipe":
        """KittiDescriptorLoader (kitti/options_descriptor.py): N/4 FPS candidates, node_num nodes, one augment scale
        U(0.9, 1.1) per pair, sn = columns 3..3+Cs, every scan at least N rows, positive_radius_threshold 5 m,
        negative_radius_threshold 50 m."""
        g = lambda k, d: getattr(opt, k, d)   # noqa: E731
        N = int(g("input_pc_num", 16384))
        return cls(N=N, M=int(g("node_num", 256)), Cs=int(g("surface_normal_len", 4)), n_sub=int(N / 4),
                   rot_horizontal=int(bool(g("rot_horizontal", True))), rot_3d=int(bool(g("rot_3d", False))),
                   rot_perturbation=int(bool(g("rot_perturbation", False))),
                   translation_perturbation=int(bool(g("translation_perturbation", False))),
                   positive_radius=float(g("positive_radius_threshold", 5.0)),
                   negative_radius=float(g("negative_radius_threshold", 50.0)))

    def c_struct(self, train: bool) -> ops.DescPairsRecipeC:
        r = ops.DescPairsRecipeC()
        for k in ("N", "M", "Cs", "n_sub", "row_len", "rot_horizontal", "rot_3d", "rot_perturbation",
                  "translation_perturbation", "aug_scale_lo", "aug_scale_hi", "shift_range", "pc_sigma", "pc_clip",
                  "sn_sigma", "sn_clip", "node_sigma", "node_clip", "pert_sigma", "pert_clip"):
            setattr(r.cloud, k, getattr(self, k))
        r.cloud.train, r.cloud.require_full = int(bool(train)), 1
        r.positive_radius, r.negative_radius, r.mine = self.positive_radius, self.negative_radius, int(self.mine)
        return r


def load_pose(p) -> np.ndarray:
    """A 4x4 pose: an array, an .npz with 'pose' (the reference's files) or an .npy."""
    if isinstance(p, (str, os.PathLike)):
        a = np.load(p)
        p = a["pose"] if hasattr(a, "files") else a
    p = np.asarray(p, dtype=np.float64)
    if p.shape != (4, 4):
        raise ValueError("PosedScanBank: a pose must be 4x4, got %s" % (p.shape,))
    return p


def sequence_layout(seq: Sequence, lengths: Sequence[int], names: Sequence[str], min_points: int):
    """seq: every scan's sequence label.  Returns (seq_of i32 [S] = index of the scan's sequence, seq_start i32
    [num_seq + 1], the labels in order).  The scans of a sequence must be contiguous (and in trajectory order: the
    positive search walks the index); a scan shorter than min_points is refused by name."""
    short = ["%s (%d rows)" % (n, l) for n, l in zip(names, lengths) if l < min_points]
    if short:
        raise ValueError("PosedScanBank: every scan needs at least N = %d rows (rows are drawn without replacement); "
                         "too short: %s" % (min_points, ", ".join(short)))
    seq = list(np.asarray(seq).reshape(-1).tolist())
    if len(seq) != len(lengths) or not seq:
        raise ValueError("PosedScanBank: %d sequence labels for %d scans" % (len(seq), len(lengths)))
    labels, starts, seq_of = [], [], []
    for i, s in enumerate(seq):
        if not labels or s != labels[-1]:
            if s in labels:
                raise ValueError("PosedScanBank: the scans of sequence %r are not contiguous (scan %d: %s)"
                                 % (s, i, names[i]))
            labels.append(s)
            starts.append(i)
        seq_of.append(len(labels) - 1)
    return (np.asarray(seq_of, dtype=np.int32), np.ascontiguousarray(starts + [len(seq)], dtype=np.int32), labels)


def _names(scans):
    return [str(s) if isinstance(s, (str, os.PathLike)) else "scan %d" % i for i, s in enumerate(scans)]


class PosedScanBank(ScanBank):
    """A ScanBank whose scans carry a pose and a sequence: poses f64 [S, 4, 4] (as the .npz files hold them) and the
    sequence layout on the device.  No radius filter (the descriptor loader has none)."""

    def __init__(self, scans: Sequence, poses: Sequence, seq: Sequence, device, min_points: int = 0, row_len: int = 8,
                 reserve: float = 0.1):
        scans = list(scans)
        lengths = [(np.load(s, mmap_mode="r") if isinstance(s, (str, os.PathLike)) else s).shape[0] for s in scans]
        meta = sequence_layout(seq, lengths, _names(scans), min_points)
        super().__init__(scans, device, row_len=row_len, radius_threshold=100.0, reserve=reserve)
        self._set_poses(poses, meta)

    def _set_poses(self, poses, meta):
        self.seq_of_host, self.seq_start_host, self.seq_labels = meta
        if isinstance(poses, torch.Tensor):
            host = poses.detach().cpu().numpy().astype(np.float64)
        else:
            host = np.stack([load_pose(p) for p in poses]) if len(poses) else np.zeros((0, 4, 4))
        if host.shape != (self.num_scans, 4, 4):
            raise ValueError("PosedScanBank: %s poses for %d scans" % (host.shape, self.num_scans))
        self.poses_host = np.ascontiguousarray(host)
        self.poses = torch.from_numpy(self.poses_host).to(self.device)
        self.seq_of = torch.from_numpy(self.seq_of_host).to(self.device)
        self.seq_start = torch.from_numpy(self.seq_start_host).to(self.device)
        self.num_seq = len(self.seq_labels)

    @classmethod
    def from_sequences(cls, sequences: Mapping, device, **kw) -> "PosedScanBank":
        """sequences: {label: (scan paths or arrays in trajectory order, poses [n, 4, 4] or pose paths)}."""
        scans, poses, seq = [], [], []
        for label, (sc, po) in sequences.items():
            sc = list(sc)
            if len(po) != len(sc):
                raise ValueError("PosedScanBank: sequence %r has %d scans and %d poses" % (label, len(sc), len(po)))
            scans += sc
            poses += [po[i] for i in range(len(sc))]
            seq += [label] * len(sc)
        return cls(scans, poses, seq, device, **kw)

    @classmethod
    def from_device_rows(cls, scans: Sequence[torch.Tensor], poses, seq, device=None, min_points: int = 0,
                         row_len: int = 8) -> "PosedScanBank":
        """The bank of float32 [rows, row_len] tensors already in device memory (usip_amd.prepare's output)."""
        scans = list(scans)
        meta = sequence_layout(seq, [int(t.shape[0]) for t in scans], _names(scans), min_points)
        self = super().from_device_rows(scans, device=device, row_len=row_len, radius_threshold=100.0)
        self._set_poses(poses, meta)
        return self

    def c_dict(self) -> dict:
        """What ops.desc_pairs_build takes as `bank`."""
        return dict(rows=self.rows, offsets=self.offsets, poses=self.poses, seq_of=self.seq_of, seq_start=self.seq_start,
                    seq_start_host=self.seq_start_host, min_rows=self.min_rows)


def synthetic_sequences(num_seq: int = 2, scans: int = 40, rows: int = 20480, spacing: float = 0.8, seed: int = 0,
                        sensor_range: float = 50.0) -> Dict[int, tuple]:
    """{sequence: ([scans] float32 [rows, 8], poses f64 [scans, 4, 4])}: one synthetic scene per sequence (a slab of points
    with unit normals, curvature and reflectance, the reference's Nx8 layout), seen from a straight-ish trajectory at
    ~`spacing` metres with a slowly turning heading.  Scan i holds `rows` scene points within sensor_range of the sensor,
    moved into the sensor frame by the inverse pose, so neighbouring scans overlap as real ones do."""
    from . import synth
    out = {}
    for q in range(num_seq):
        rng = np.random.default_rng([int(seed), q])
        length = spacing * (scans - 1)
        # the slab is 100 m wide in z: 1.5x the density that puts `rows` points into a disc of sensor_range
        n_scene = int(1.5 * rows * (length + 2 * sensor_range) * 100.0 / (np.pi * sensor_range ** 2)) + rows
        world = synth.make_cloud(rng, n_scene, "slab").T.astype(np.float64)           # x, z in [-50, 50], y thin
        world[:, 0] = rng.uniform(-sensor_range, length + sensor_range, n_scene)
        extra = synth.make_normals(rng, n_scene, 5).T.astype(np.float64)              # nx ny nz curvature reflectance
        clouds, poses = [], []
        for i in range(scans):
            yaw = 0.01 * i + rng.normal(0, 0.002)                                     # about y, the camera frame's up
            c, s = np.cos(yaw), np.sin(yaw)
            P = np.eye(4)
            P[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
            P[:3, 3] = [spacing * i + rng.normal(0, 0.02), rng.normal(0, 0.01), rng.normal(0, 0.05)]
            near = np.flatnonzero(np.hypot(world[:, 0] - P[0, 3], world[:, 2] - P[2, 3]) <= sensor_range)
            if near.size < rows:
                raise ValueError("synthetic_sequences: %d scene points in range, %d rows asked for" % (near.size, rows))
            pick = rng.choice(near, rows, replace=False)
            R = P[:3, :3]
            local = (world[pick] - P[:3, 3]) @ R                                      # R' (p - t) as row vectors
            clouds.append(np.concatenate([local, extra[pick, :3] @ R, extra[pick, 3:]], 1).astype(np.float32))
            poses.append(P)
        out[q] = (clouds, np.stack(poses))
    return out


def empty_batch(c: ops.DescPairsRecipeC, pairs: int, device) -> Dict[str, torch.Tensor]:
    """Every build writes every float; neg_idx / neg_fail are written only when the recipe mines, so they start at 0."""
    return _empty_batch(ops.DESC_PAIRS, c, pairs, device)


class DescriptorPairBuilder(_CloudBuilder):
    """P (anchor, positive) pairs per call, with the negatives mined among the call's own P anchors.

    Negatives are mined within the rank's own P pairs: data parallel shards the pairs, as everywhere in this project,
    so rank r's neg_idx indexes rank r's anchors (the reference mines within one DataLoader batch in the same way).
    A pair's clouds and positive depend on (seed, step, rank * P + p) only; its negative also on the other P - 1 anchors.

    build(scan_ids, step, out=None): Philox draws.  `out` may hold any of KEYS (e.g. the anc_pc, pos_pc, anc_sn, pos_sn,
        neg_idx buffers of DescriptorStep.static_batch), which are then written in place; the rest is allocated.
    apply(scan_ids, draws, out=None): the recorded draws of the reference (tests).
    prefetch(schedule): double-buffered, batch k+1 built on a side stream while the consumer runs batch k.
    build / apply use one workspace, each prefetch buffer one of its own."""

    spec = ops.DESC_PAIRS

    def _check(self):
        if self.bank.min_rows < self.recipe.N:
            raise ValueError("DescriptorPairBuilder: every scan needs at least N = %d rows; the bank's shortest has %d"
                             % (self.recipe.N, self.bank.min_rows))
        if self.recipe.mine and self.pairs < 2:
            raise ValueError("DescriptorPairBuilder: mining negatives needs at least 2 pairs per call")


def build_cpu(recipe: DescriptorPairRecipe, scans: Sequence[np.ndarray], poses, seq, scan_ids, pairs: int, seed: int = 0,
              step: int = 0, rank: int = 0, mode: str = "train", draws: Optional[Dict[str, np.ndarray]] = None):
    """The host twin (usip_desc_pairs_build_f32_cpu) on numpy scans and poses [S, 4, 4]: Philox draws, or `draws` (the
    layouts of include/usip_hip.h).  Returns (batch, rows [2,P,N], node_slots [2,P,M]).  The same refusals as the bank's."""
    scans = [np.asarray(s, dtype=np.float32) for s in scans]
    seq_of, seq_start, _ = sequence_layout(seq, [len(s) for s in scans], _names(scans), recipe.N)
    poses = np.ascontiguousarray(np.stack([load_pose(p) for p in poses]))
    if poses.shape[0] != len(scans):
        raise ValueError("build_cpu: %d poses for %d scans" % (poses.shape[0], len(scans)))
    return host_twin(ops.DESC_PAIRS, lambda row_len: recipe.c_struct(mode == "train"), scans, "scan", scan_ids, pairs,
                     bank=dict(poses=poses, seq_of=seq_of, seq_start=seq_start, seq_start_host=seq_start),
                     counter=(seed, step, rank * int(pairs)), draws=draws)


class _FrozenDetectorTrainer:
    """What DescriptorTrainer and indoor_pairs.IndoorDescriptorTrainer share: the frozen eval-mode detector that gives every
    built batch its keypoints and sigmas, the descriptor step made under torch.manual_seed(seed), the point permutation
    drawn ON THE DEVICE from the seed, and the checkpoint gate.  A trainer supplies _make_step and its own batches."""

    def __init__(self, builder, detector_model: str, detector_state, opt, device=None, seed: int = 0, graph: bool = False,
                 min_save_epoch: int = 0, with_optimizer: bool = True):
        from . import inference
        from .networks import build_detector
        self.builder, self.opt = builder, opt
        self.device = torch.device(device) if device is not None else builder.device
        self.detector = build_detector(detector_model, opt).to(self.device)
        inference.load_detector_state(self.detector, detector_state)
        for p in self.detector.parameters():                  # freeze_model
            p.requires_grad = False
        self.detector.eval()
        torch.manual_seed(int(seed))
        self.st = self._make_step(opt, with_optimizer, graph, int(seed))
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self.best_loss, self.min_save_epoch = 1e6, int(min_save_epoch)
        self.last_loss = self.last_active = None

    def _keypoints(self, batch: Dict[str, torch.Tensor]):
        """run_model_siamese on cat(anchor, positive), and the permutation: (P, keypoints [2P,3,M], sigmas [2P,M], perm)."""
        from . import inference
        P, N = batch["anc_pc"].shape[0], batch["anc_pc"].shape[2]
        kp, sg = inference.run_model(self.detector, torch.cat((batch["anc_pc"], batch["pos_pc"]), 0),
                                     torch.cat((batch["anc_sn"], batch["pos_sn"]), 0),
                                     torch.cat((batch["anc_node"], batch["pos_node"]), 0))
        return P, kp, sg, torch.randperm(N, generator=self._gen, device=self.device)

    def _save_due(self, test_loss: float, epoch: int) -> bool:
        return test_loss <= self.best_loss + 1e-5 and epoch >= self.min_save_epoch

    def save_if_best(self, path: str, test_loss: float, epoch: int = 0) -> bool:
        """The checkpoint (descriptor.state_dict(), the reference's keys) is written when the test loss is the best so far
        and the epoch has reached min_save_epoch (the reference: half an lr_decay_step)."""
        if test_loss <= self.best_loss:
            self.best_loss = test_loss
        if self._save_due(test_loss, epoch):
            torch.save(self.st.descriptor.state_dict(), path)
            return True
        return False


class DescriptorTrainer(_FrozenDetectorTrainer):
    """kitti/train_descriptor.py:69-212 on one device: a frozen detector gives the keypoints and sigmas of every built
    batch, DescriptorStep trains on them, a test pass gates the checkpoint.

    Per train_step(batch): eval-mode no-grad detector forward on cat(anchor, positive) (run_model_siamese), anc_kp, pos_kp
    and anc_sigmas from it, the point permutation DescriptorStep needs drawn ON THE DEVICE from the seed, then
    DescriptorStep.step.  Everything is enqueued on the current stream and nothing is read back; neg_fail_total (device
    i32 [1]) accumulates the batches' neg_fail, last_loss / last_active are device tensors.
    The descriptor is initialised under torch.manual_seed(seed): the same seed gives the same run, bit for bit."""

    def __init__(self, builder: DescriptorPairBuilder, detector_model: str, detector_state, opt, device=None,
                 seed: int = 0, graph: bool = False, min_save_epoch: int = 0, with_optimizer: bool = True):
        super().__init__(builder, detector_model, detector_state, opt, device, seed, graph, min_save_epoch, with_optimizer)
        self.neg_fail_total = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _make_step(self, opt, with_optimizer, graph, seed):
        from .step import DescriptorStep
        return DescriptorStep(opt, self.device, with_optimizer=with_optimizer, graph=graph)

    def descriptor_batch(self, batch: Dict[str, torch.Tensor], out: Optional[Dict[str, torch.Tensor]] = None):
        """The builder's batch -> what DescriptorStep consumes; with `out` (DescriptorStep.static_batch) the keypoints,
        sigmas and permutation are written into it."""
        P, kp, sg, perm = self._keypoints(batch)
        d = dict(anc_pc=batch["anc_pc"], pos_pc=batch["pos_pc"], anc_sn=batch["anc_sn"], pos_sn=batch["pos_sn"],
                 anc_kp=kp[:P].contiguous(), pos_kp=kp[P:].contiguous(), anc_sigmas=sg[:P].contiguous(),
                 neg_idx=batch["neg_idx"], perm=perm)
        if out is not None:
            for k in ("anc_kp", "pos_kp", "anc_sigmas", "perm"):
                out[k].copy_(d[k])
                d[k] = out[k]
        return d

    def train_step(self, batch: Dict[str, torch.Tensor], epoch: Optional[int] = None, group=None, out=None):
        loss = self.st.step(self.descriptor_batch(batch, out), epoch=epoch, group=group)
        self.neg_fail_total += batch["neg_fail"]
        self.last_loss, self.last_active = loss, self.st.last["active"]
        return loss

    def test_pass(self, test_builder: DescriptorPairBuilder, schedule: Iterable):
        """train_descriptor.py:146-207: eval-mode forward and loss under no_grad on test-mode batches, averaged with the
        batch size as weight.  Returns (loss, active percentage) as floats -- the one read-back, once per pass."""
        desc = self.st.descriptor
        was_training = desc.training
        desc.eval()
        loss_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        active_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        count = 0
        try:
            with torch.no_grad():
                for ids, step in schedule:
                    d = self.descriptor_batch(test_builder.build(ids, step))
                    B = d["anc_pc"].shape[0]
                    out, _ = desc(torch.cat((d["anc_pc"], d["pos_pc"]), 0), torch.cat((d["anc_sn"], d["pos_sn"]), 0),
                                  torch.cat((d["anc_kp"], d["pos_kp"]), 0), False, None, perm=d["perm"])
                    anc, pos = torch.split(out, B, dim=0)
                    triplet, active = self.st.triplet_criteria(anc, pos, anc[d["neg_idx"], :, :], d["anc_sigmas"])
                    loss_sum += torch.mean(triplet) * B
                    active_sum += torch.mean(active) * B
                    count += B
        finally:
            desc.train(was_training)
        if count == 0:
            raise ValueError("DescriptorTrainer.test_pass: an empty schedule")
        return float(loss_sum) / count, float(active_sum) / count
