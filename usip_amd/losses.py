"""Detector losses with the reference's class names and call signatures (models/losses.py),
built on the fused nearest-neighbour kernel instead of materialised B x M x N matrices
(SURVEY 8 a-9, a-10)."""
import torch
import torch.nn as nn

from . import functional as Fh


class ChamferLoss_Brute(nn.Module):
    """Probabilistic (sigma-weighted) chamfer loss (models/losses.py:44-99).
    forward(src Bx3xM, dst Bx3xN, sigma_src BxM, sigma_dst BxN) -> (loss, chamfer_pure, chamfer_weighted)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.dimension = 3

    def forward(self, pc_src_input, pc_dst_input, sigma_src=None, sigma_dst=None):
        a, J = Fh.nearest_distance_i32(pc_src_input, pc_dst_input)      # row minima  (:81)
        c, I = Fh.nearest_distance_i32(pc_dst_input, pc_src_input)      # column minima (:86)
        self.last_indices = (J, I)                                       # int32 (torch.min gives int64)
        if sigma_src is None or sigma_dst is None:                       # losses.py:68-78
            return a + c, a + c, a + c
        return Fh.chamfer_prob(a, J, c, I, sigma_src, sigma_dst)         # :82-99, one launch


class SingleSideChamferLoss_Brute(nn.Module):
    """min_n |src[b,:,m] - dst[b,:,n]| -> BxM (models/losses.py:119-143)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.dimension = 3

    def forward(self, pc_src_input, pc_dst_input, grid=None):
        return Fh.nearest_distance_i32(pc_src_input, pc_dst_input, grid)[0]


class PointOnSurfaceLoss(nn.Module):
    """Point-to-plane form (models/losses.py:146-187): with p = the cloud point nearest to the keypoint and n its
    normal (the first three channels of sn), (n . (kp - p) / (|kp - p| + 1e-7))^2 -> B x M x 1 x 1.  The arg-min comes
    from the fused nearest-neighbour kernel (no B x M x N matrix); the rest is M-sized ATen arithmetic in the
    reference's order, which autograd differentiates exactly as it does there (the arg-min carries no gradient)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt

    def forward(self, keypoint, pc, sn):
        B, M = keypoint.shape[0], keypoint.shape[2]
        _, I = Fh.nearest_distance_i32(keypoint.detach(), pc)
        self.last_indices = I
        idx = I.long().unsqueeze(1).expand(B, 3, M)
        pc_selected = torch.gather(pc, 2, idx)
        sn_selected = torch.gather(sn, 2, idx)                          # channels 0..2 of sn
        diff = keypoint - pc_selected
        unit = diff / (torch.norm(diff, dim=1, keepdim=True) + 1e-7)
        dot = torch.matmul(sn_selected.permute(0, 2, 1).unsqueeze(2), unit.permute(0, 2, 1).unsqueeze(3))
        return dot ** 2                                                 # B x M x 1 x 1


class KeypointOnPCLoss(nn.Module):
    """Keypoint-to-cloud distance (models/losses.py:102-116): point-to-point (sn None: the default of every options
    file) or point-to-plane (sn given; selected by opt.keypoint_on_pc_type, keypoint_detector.py:193-201)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.single_side_chamfer = SingleSideChamferLoss_Brute(opt)
        self.keypoint_on_surface = PointOnSurfaceLoss(opt)

    def forward(self, keypoint, pc, sn=None, grid=None):
        """grid: an ops.CellGrid built from pc; the point-to-point distances then come through it (same values)."""
        if sn is not None:
            return self.keypoint_on_surface(keypoint, pc, sn)
        return self.single_side_chamfer(keypoint, pc, grid)


class DescPairScanLoss(nn.Module):
    """Descriptor triplet loss with in-batch negatives (models/losses.py:190-237):
    for every anchor keypoint the nearest positive-scan and nearest negative-scan descriptor,
    clamp(d_pos - d_neg + gamma, 0) weighted by clamp(sigma_max - sigma, 0) normalised to mean 1.
    forward(anc BxCxM, pos BxCxM, neg BxCxM, anc_sigmas BxM) -> (loss BxM, active_percentage B).
    The two B x C x M x M difference tensors of the reference are replaced by the fused nearest kernel."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt

    def forward(self, anc_descriptors, pos_descriptors, neg_descriptors, anc_sigmas):
        d_pos, j_pos = Fh.nearest_distance_i32(anc_descriptors, pos_descriptors)
        d_neg, j_neg = Fh.nearest_distance_i32(anc_descriptors, neg_descriptors)
        self.last_indices = (j_pos, j_neg)                              # int32 (torch.min gives int64)
        before_clamp = d_pos - d_neg + self.opt.triple_loss_gamma
        active_percentage = torch.mean((before_clamp > 0).float(), dim=1)
        w = torch.clamp(self.opt.sigma_max - anc_sigmas, min=0)
        w = (w / torch.mean(w, dim=1, keepdim=True)).detach()
        return w * torch.clamp(before_clamp, min=0), active_percentage


class DescCGFLoss(nn.Module):
    """The indoor descriptor's CGF triplet loss (models/losses.py:240-314): for every anchor keypoint a random
    positive keypoint within opt.CGF_radius and, with equal odds, the nearest keypoint beyond the radius or a random one
    beyond it; clamp(d_pos - d_neg + opt.triple_loss_gamma, 0) over the matched anchors, rescaled by M / (matched + 1) and
    weighted by clamp(opt.sigma_max - sigma, 0) normalised to mean 1.
    forward(anc_keypoints Bx3xM (in the positive's frame), anc_descriptors BxCxM, pos_keypoints Bx3xM, pos_descriptors BxCxM,
    anc_sigmas BxM, anc_pc=None, pos_pc=None) -> (loss BxM, active_percentage B).  anc_pc and pos_pc are accepted and ignored
    (the reference reads them in commented-out code only).  The reference's B x C x M x M difference tensor and its three
    random B x M x M matrices are replaced by the fused selection and distance kernels.  When every sigma of a batch element
    is at or above sigma_max the reference returns NaN (0 / 0); here that row is 0.

    Random numbers: counter-based (Philox) from (seed, step, batch element, i, j).  Keyword-only additions: seed at
    construction; on the call draws = dict(u1, u2 f32 BxMxM, u3 f32 BxM) for recorded uniforms, and step = an int or a
    one-element int64 device tensor.  By default an internal device word is the step and is incremented in-stream after each
    call in training mode, so a captured graph draws fresh numbers on every replay.  last_indices = (sel i32 BxMx3 =
    (j_pos, j_far, j_out), has u8 BxM, take_far u8 BxM).  Host tensors go to the host twin."""

    def __init__(self, opt, *, seed: int = 0):
        super().__init__()
        self.opt = opt
        self.seed = int(seed)
        self._step_dev = None                                           # one int64 word per device, made on first use
        self._step_host = 0

    def _step(self, device):
        if device.type != "cuda":
            return self._step_host
        if self._step_dev is None or self._step_dev.device != device:
            self._step_dev = torch.full((1,), self._step_host, dtype=torch.int64, device=device)
        return self._step_dev

    def forward(self, anc_keypoints, anc_descriptors, pos_keypoints, pos_descriptors, anc_sigmas, anc_pc=None, pos_pc=None, *,
                draws=None, step=None):
        own = step is None and draws is None
        if step is None:
            step = self._step(anc_descriptors.device) if own else 0
        loss, active, sel, has, take_far = Fh.cgf_triplet(
            anc_keypoints, anc_descriptors, pos_keypoints, pos_descriptors, anc_sigmas, self.opt.CGF_radius,
            self.opt.triple_loss_gamma, self.opt.sigma_max, draws, self.seed, step)
        self.last_indices = (sel, has, take_far)
        if own and self.training:
            if isinstance(step, torch.Tensor):
                step.add_(1)                                            # in-stream: behind the selection that read it
            else:
                self._step_host += 1
        return loss, active
