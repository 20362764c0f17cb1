"""Training pairs built on the GPU from device-resident scans.

The reference builds every (src, dst) pair on the CPU in DataLoader workers (KittiLoader / OxfordLoader.__getitem__,
data/kitti_detector_loader.py:101-259, data/oxford_detector_loader.py:99-229, data/augmentation.py:199-248).  Here the
scans live in HBM (ScanBank) and one call enqueues the whole batch -- subsampling, FPS nodes, augment and the dst
transform -- on the current stream, with no host synchronisation (csrc/pairs.hip):

    bank = ScanBank.from_paths(sorted(glob.glob("seq/*.npy")), "cuda:0", radius_threshold=opt.radius_threshold)
    builder = PairBuilder(bank, PairRecipe.kitti(opt), pairs=8, device="cuda:0", seed=0, rank=rank)
    for step, ids in enumerate(epoch_batches(bank.num_scans, 8, seed=0, epoch=0, rank=rank, world=world)):
        st.step(builder.build(ids, step))

Randomness is Philox4x64-10 keyed by the seed, with counter (element, stream, rank * P + p, step): a pair's data does not
depend on the world size, and the same (seed, step, pair) always gives the same batch.
"""
import ctypes
import os
from dataclasses import dataclass, fields
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

KEYS = ops.PAIRS_KEYS


@dataclass
class PairRecipe:
    """What one pair is made of: the fields of usip_pairs_recipe (include/usip_hip.h) bar `train`, which the builder's
    mode sets.  Built by the presets below from the reference's option names and defaults."""
    N: int = 16384
    M: int = 512
    Cs: int = 4
    n_sub: int = 5461
    row_len: int = 8
    sn_last: int = 0
    rot_horizontal: int = 1
    rot_3d: int = 0
    rot_perturbation: int = 0
    translation_perturbation: int = 0
    height_scaling: int = 0
    enu_to_cam: int = 0
    require_full: int = 0
    dst_rot_type: int = 2
    dst_rot_perturbation: int = 0
    aug_scale_lo: float = 0.9
    aug_scale_hi: float = 1.1
    shift_range: float = 1.0
    height_lo: float = 0.25
    height_hi: float = 1.2
    pc_sigma: float = 0.04
    pc_clip: float = 0.12
    sn_sigma: float = 0.01
    sn_clip: float = 0.05
    node_sigma: float = 0.04
    node_clip: float = 0.12
    pert_sigma: float = 0.06
    pert_clip: float = 0.18
    dst_scale_thre: float = 0.0
    dst_shift_thre: float = 0.5
    radius_threshold: float = 100.0          # applied once, by ScanBank (KITTI: rows with xz norm <= r when r < 90)

    @staticmethod
    def _common(opt):
        g = lambda k, d: getattr(opt, k, d)   # noqa: E731
        rot_3d, rot_h, pert = bool(g("rot_3d", False)), bool(g("rot_horizontal", True)), bool(g("rot_perturbation", False))
        return dict(N=int(g("input_pc_num", 16384)), M=int(g("node_num", 512)), Cs=int(g("surface_normal_len", 4)),
                    rot_horizontal=int(rot_h), rot_3d=int(rot_3d), rot_perturbation=int(pert),
                    translation_perturbation=int(bool(g("translation_perturbation", False))),
                    dst_rot_type=3 if rot_3d else (2 if rot_h else 0), dst_rot_perturbation=int(pert))

    @classmethod
    def kitti(cls, opt) -> "PairRecipe":
        """KittiLoader (kitti/options_detector.py): N/3 FPS candidates, augment scale U(0.9, 1.1), Cs == 1 takes the
        row's last column, scans shorter than N take the fix_idx layout, radius_threshold < 90 filters rows."""
        kw = cls._common(opt)
        return cls(n_sub=int(kw["N"] / 3), sn_last=int(kw["Cs"] == 1), aug_scale_lo=0.9, aug_scale_hi=1.1,
                   radius_threshold=float(getattr(opt, "radius_threshold", 100.0)), **kw)

    @classmethod
    def oxford(cls, opt) -> "PairRecipe":
        """OxfordLoader (oxford/options_detector.py): N/8 candidates, height scaling U(0.25, 1.2) of ENU z before FPS
        (train mode), coordinate_ENU_to_cam after it (Cs >= 3), augment scale U(0.7, 1.3), scans of at least N rows."""
        kw = cls._common(opt)
        if kw["Cs"] < 3:
            raise ValueError("PairRecipe.oxford: coordinate_ENU_to_cam permutes sn columns 0-2, surface_normal_len >= 3")
        return cls(n_sub=int(kw["N"] / 8), height_scaling=int(bool(getattr(opt, "is_height_scaling", True))),
                   enu_to_cam=1, require_full=1, aug_scale_lo=0.7, aug_scale_hi=1.3, **kw)

    def c_struct(self, train: bool) -> ops.PairsRecipeC:
        r = ops.PairsRecipeC()
        for f in fields(self):
            if f.name != "radius_threshold":
                setattr(r, f.name, getattr(self, f.name))
        r.train = int(bool(train))
        return r


class ScanBank:
    """All scans in ONE float32 device buffer [rows, row_len] plus int64 row offsets (CSR): scan s is rows
    offsets[s] .. offsets[s+1].  A float64 scan is rounded to float32 here; KITTI's radius filter (a deterministic
    function of the file) is applied here, once, on the values as the file holds them.  A scan the filter empties is
    refused by name."""

    def __init__(self, scans: Sequence, device, row_len: int = 8, radius_threshold: float = 100.0, reserve: float = 0.1):
        self.device = torch.device(device)
        arrays = []
        for s in scans:
            a = np.load(s, mmap_mode="r") if isinstance(s, (str, os.PathLike)) else s
            a = np.asarray(a)
            if a.ndim != 2 or a.shape[1] != row_len:
                raise ValueError("ScanBank: a scan must be [rows, %d], got %s" % (row_len, a.shape))
            arrays.append(a)
        if not arrays:
            raise ValueError("ScanBank: no scans")
        masks = []
        for a in arrays:
            if radius_threshold < 90:       # in the file's own dtype, as the reference computes it (before rounding)
                masks.append(np.linalg.norm(np.asarray(a[:, [0, 2]]), axis=1) <= radius_threshold)
            else:
                masks.append(None)
        lengths = np.array([a.shape[0] if m is None else int(m.sum()) for a, m in zip(arrays, masks)], dtype=np.int64)
        empty = [(s if not isinstance(s, np.ndarray) else "scan %d" % i) for i, s in enumerate(scans) if lengths[i] == 0]
        if empty:
            raise ValueError("ScanBank: no rows left in %s (radius_threshold %g)" % (", ".join(map(str, empty)),
                                                                                    radius_threshold))
        self.lengths = lengths
        self.offsets_host = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        total = int(self.offsets_host[-1]) * row_len * 4
        free, _ = torch.cuda.mem_get_info(self.device)
        if total > (1.0 - reserve) * free:
            raise MemoryError("ScanBank: %d scans need %.2f GB of device memory, %s has %.2f GB free (keeping %d%% for "
                              "the step)" % (len(arrays), total / 1e9, self.device, free / 1e9, int(100 * reserve)))
        self.rows = torch.empty((int(self.offsets_host[-1]), row_len), dtype=torch.float32, device=self.device)
        for s, (a, m) in enumerate(zip(arrays, masks)):
            if lengths[s]:
                h = np.ascontiguousarray(a if m is None else a[m], dtype=np.float32)
                self.rows[self.offsets_host[s]:self.offsets_host[s + 1]].copy_(torch.from_numpy(h))
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.row_len = row_len
        self.num_scans = len(arrays)
        self.min_rows = int(lengths.min())

    @classmethod
    def from_paths(cls, paths: Sequence[str], device, **kw) -> "ScanBank":
        return cls(list(paths), device, **kw)

    @classmethod
    def from_device_rows(cls, scans: Sequence[torch.Tensor], device=None, row_len: int = 8,
                         radius_threshold: float = 100.0) -> "ScanBank":
        """The bank of float32 [rows, row_len] tensors that are already in device memory (usip_amd.prepare's output):
        the same bank as ScanBank([t.cpu().numpy() for t in scans], ...) without the trip through the host.  Only the
        row counts are read back."""
        scans = list(scans)
        if not scans:
            raise ValueError("ScanBank: no scans")
        self = cls.__new__(cls)
        self.device = torch.device(device) if device is not None else scans[0].device
        kept = []
        for i, t in enumerate(scans):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != row_len or t.dtype != torch.float32:
                raise ValueError("ScanBank: a scan must be a float32 tensor [rows, %d], got %s" % (
                    row_len, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
            t = t.to(self.device)
            if radius_threshold < 90:       # sqrt(x * x + z * z) in float32: what numpy's norm computes on the host path
                t = t[torch.sqrt(t[:, 0] * t[:, 0] + t[:, 2] * t[:, 2]) <= radius_threshold]
            if t.shape[0] == 0:
                raise ValueError("ScanBank: no rows left in scan %d (radius_threshold %g)" % (i, radius_threshold))
            kept.append(t)
        self.lengths = np.array([t.shape[0] for t in kept], dtype=np.int64)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.rows = torch.cat(kept).contiguous()
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.row_len = row_len
        self.num_scans = len(kept)
        self.min_rows = int(self.lengths.min())
        return self

    def c_dict(self) -> dict:
        """What ops.cloud_batch takes as `bank`."""
        return dict(rows=self.rows, offsets=self.offsets, min_rows=self.min_rows)


def epoch_order(num_scans: int, seed: int, epoch: int) -> np.ndarray:
    """DataLoader(shuffle=True) order of one epoch: a permutation of the scans, a function of (seed, epoch) only."""
    return np.random.default_rng([int(seed), int(epoch)]).permutation(int(num_scans)).astype(np.int32)


def epoch_batches(num_scans: int, pairs: int, seed: int, epoch: int, rank: int = 0, world: int = 1):
    """This rank's scan ids per step of one epoch, drop_last=True: global batch k = order[k*P*W : (k+1)*P*W], rank r
    takes its r-th slice of P (pair index rank * P + p, as the builder's counter uses)."""
    order = epoch_order(num_scans, seed, epoch)
    g = pairs * world
    for k in range(len(order) // g):
        yield order[k * g + rank * pairs:k * g + (rank + 1) * pairs]


def _empty_batch(spec: ops.CloudBatchSpec, c, n: int, device, skip=()) -> Dict[str, torch.Tensor]:
    """Buffers of a call of n ids, bar the keys in `skip`.  Every build writes every float; an integer output may be left
    untouched (f-8's neg_idx / neg_fail when the recipe does not mine), so those start at 0."""
    return {k: (torch.empty if dt == torch.float32 else torch.zeros)(shape, dtype=dt, device=device)
            for k, (shape, dt) in ops.cloud_batch_table(spec, c, n).items() if k not in skip}


def empty_batch(recipe: PairRecipe, pairs: int, device) -> Dict[str, torch.Tensor]:
    return _empty_batch(ops.PAIRS, recipe, pairs, device)


_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}


class _CloudBuilder:
    """What the four builders share (PairBuilder, desc_pairs.DescriptorPairBuilder, indoor_pairs.IndoorPairBuilder,
    fragment_batch.FragmentBatchBuilder): the bookkeeping, the upload of the ids, completing `out`, the optional index
    outputs, build and apply, three workspaces ([0]: build / apply, [1], [2]: the two prefetch buffers) and prefetch.
    A builder supplies its declaration `spec` (ops.CloudBatchSpec) and _check (its refusals).  pairs = 0: any number of
    ids per call (the fragment builder, which keeps its own workspaces)."""

    spec = None
    _modes = ("train", "test")

    def __init__(self, bank, recipe, pairs: int, device=None, seed: int = 0, rank: int = 0, mode: str = "train"):
        if mode not in self._modes:
            raise ValueError("%s: mode is %s" % (type(self).__name__, " or ".join(repr(m) for m in self._modes)))
        self.bank, self.recipe, self.pairs = bank, recipe, int(pairs)
        self.device = torch.device(device) if device is not None else bank.device
        self.seed, self.rank, self.mode = int(seed), int(rank), mode
        self.c = self._c_struct()
        self._check()
        self._bank, self._keys = bank.c_dict(), frozenset(self.spec.keys)
        self._ws = [torch.empty(ops.cloud_batch_workspace(self.spec, self.c, self.pairs), dtype=torch.uint8,
                                device=self.device) for _ in range(3 if self.pairs else 0)]
        self.last_rows = self.last_node_slots = None

    def _c_struct(self):
        return self.recipe.c_struct(self.mode == "train")

    def _num_ids(self) -> int:
        """What the ids of a call index: the bank's scans (the indoor builder: its samples)."""
        return self.bank.num_scans

    def _ids(self, ids, with_host: bool = False):
        """-> the ids as an i32 device tensor; with_host: (that, their int32 host copy, or None for ids already on the
        device)."""
        name, what, host = type(self).__name__, self.spec.ids, None
        if isinstance(ids, torch.Tensor) and ids.is_cuda:
            if ids.device != self.bank.device:
                raise ValueError("%s: %s ids on %s, the bank on %s" % (name, what, ids.device, self.bank.device))
            dev = ids.to(torch.int32).contiguous()
            dev = dev if dev.dim() == 1 else dev.reshape(-1)
        else:
            h = np.asarray(ids, dtype=np.int64).reshape(-1)
            if h.size and (h.min() < 0 or h.max() >= self._num_ids()):
                raise ValueError("%s: %s id out of range [0, %d)" % (name, what, self._num_ids()))
            host = np.ascontiguousarray(h, dtype=np.int32)
            dev = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
        n = dev.numel()
        if self.pairs and n != self.pairs:
            raise ValueError("%s: %d %s ids for %d pairs" % (name, n, what, self.pairs))
        if n < 1:
            raise ValueError("%s: no ids" % name)
        return (dev, host) if with_host else dev

    def _empty_batch(self, n: Optional[int] = None):
        return _empty_batch(self.spec, self.c, self.pairs if n is None else n, self.device)

    def _out(self, n: int, out, with_indices):
        """(the builder's keys: those `out` holds, fresh buffers for the rest; rows, node_slots).  Every key given:
        nothing is allocated, and an `out` of exactly the keys is used as it is."""
        keys = self.spec.keys
        if out is None or out.keys() != self._keys:
            given = {} if out is None else {k: out[k] for k in keys if k in out}
            fresh = _empty_batch(self.spec, self.c, n, self.device, skip=given)
            out = {k: given[k] if k in given else fresh[k] for k in keys}
        return (out,) + self._index_out(n, with_indices)

    def _index_out(self, n: int, with_indices):
        self.last_rows = self.last_node_slots = rows = nodes = None
        if with_indices:
            lead = self.spec.index_lead(n)
            rows = torch.empty(lead + (self.recipe.N,), dtype=torch.int32, device=self.device)
            nodes = torch.empty(lead + (self.recipe.M,), dtype=torch.int32, device=self.device)
            self.last_rows, self.last_node_slots = self._of_call(dict(rows=rows, nodes=nodes), n).values()
        return rows, nodes

    def _of_call(self, tensors: dict, n: int) -> dict:
        """What a call of n ids hands back of the buffers it filled (the fragment builder: their first n clouds)."""
        return tensors

    def _workspace(self, n: int, which: int = 0) -> torch.Tensor:
        return self._ws[which]

    def _counter(self, step: int) -> tuple:
        return (self.seed, int(step), self.rank * self.pairs)

    def _run(self, ids, out, with_indices, which, counter=None, draws=None):
        ids, host = self._ids(ids, with_host=True)
        n = ids.numel()
        out, rows, nodes = self._out(n, out, with_indices)
        ops.cloud_batch(self.spec, self.c, self._bank, ids, out, self._workspace(n, which), rows, nodes, counter, draws,
                        host)
        return self._of_call(out, n)

    def build(self, ids, step: int, out: Optional[Dict[str, torch.Tensor]] = None, with_indices: bool = False,
              _ws: int = 0) -> Dict[str, torch.Tensor]:
        """Philox draws under (seed, step); `out` may hold any of the builder's KEYS, which are then written in place."""
        return self._run(ids, out, with_indices, _ws, counter=self._counter(step))

    def apply(self, ids, draws: Dict[str, np.ndarray], out=None, with_indices: bool = True):
        """The recorded draws of the reference (tests), as arrays in the header's layouts: held to them before any is
        uploaded."""
        h = {k: np.ascontiguousarray(draws[k], dtype=_NP[dt]) for k, dt in self.spec.draws.items()
             if draws.get(k) is not None}
        ops.check_draws(self.spec, ops.cloud_recipe(self.c), ids.numel() if isinstance(ids, torch.Tensor) else np.size(ids),
                        h, ValueError)
        return self._run(ids, out, with_indices, 0, draws={k: torch.from_numpy(a).to(self.device) for k, a in h.items()})

    def workspace_candidates(self, which: int = 0):
        """The un-augmented FPS candidates [2P, 3, n_sub] and first indices [2P] in workspace `which` (0: the last build
        or apply), at the offsets the library reports (usip_pairs_workspace_offset, usip_desc_pairs_workspace_offset)."""
        P, ns = self.pairs, self.recipe.n_sub
        ws = self._ws[which]
        o_c, o_f = (ops.cloud_batch_workspace(self.spec, self.c, P, part) for part in (1, 2))
        cand = ws[o_c:o_c + 2 * P * 3 * ns * 4].view(torch.float32).view(2 * P, 3, ns)
        first = ws[o_f:o_f + 2 * P * 4].view(torch.int32)
        return cand, first

    def prefetch(self, schedule: Iterable, outs=None):
        """schedule: iterable of (scan_ids, step).  Yields each batch on the current stream's order; while the consumer
        enqueues work on batch k, batch k+1 is built on a side stream into the other buffer.  Events order everything:
        the consumer's stream waits for 'built', the side stream for 'consumed'; the host never waits.

        Leaving the loop early (break, an exception, closing the generator) is safe: when the generator ends, the
        current stream waits for every build still in flight on the side stream, so later work on the current stream --
        reusing `outs`, or memory the allocator hands out again -- is ordered after the last write.  The internal
        buffers are also marked as used on the side stream, so the allocator does not reuse them before it is done.
        A yielded batch is valid until the next iteration (it is rebuilt two batches later)."""
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(self.device)
        if outs is None:
            bufs = [self._empty_batch() for _ in range(2)]
            for b in bufs:
                for t in b.values():
                    t.record_stream(side)
        else:
            bufs = outs
        built = [torch.cuda.Event(), torch.cuda.Event()]
        consumed = [None, None]

        def enqueue(i, ids, step):
            if consumed[i] is not None:
                side.wait_event(consumed[i])
            else:
                side.wait_stream(cur)
            with torch.cuda.stream(side):
                self.build(ids, step, out=bufs[i], _ws=1 + i)
            built[i].record(side)

        try:
            it = iter(schedule)
            nxt = next(it, None)
            if nxt is None:
                return
            enqueue(0, *nxt)
            k = 0
            while True:
                nxt = next(it, None)
                if nxt is not None:
                    enqueue((k + 1) % 2, *nxt)
                cur.wait_event(built[k % 2])
                yield bufs[k % 2]
                ev = torch.cuda.Event()
                ev.record(cur)
                consumed[k % 2] = ev
                k += 1
                if nxt is None:
                    return
        finally:
            cur.wait_stream(side)


class PairBuilder(_CloudBuilder):
    """P pairs per call, written as DetectorStep.step consumes them (synth.make_pair_batch's shapes and dtypes).

    build(scan_ids, step, out=None): Philox draws; `out` (e.g. st.static_batch(batch)) is written in place.
    apply(scan_ids, draws, out=None): the recorded draws of the reference (tests).
    prefetch(schedule): double-buffered, batch k+1 built on a side stream while the consumer runs batch k.
    build / apply use one workspace, each prefetch buffer one of its own, so a build on the current stream never races
    a live prefetch; two builds on two different streams at once are the caller's to order."""

    epoch_order = staticmethod(epoch_order)
    spec = ops.PAIRS

    def _check(self):
        if self.recipe.require_full and self.bank.min_rows < self.recipe.N:
            raise ValueError("PairBuilder: this recipe needs scans of at least N = %d rows; the bank's shortest has %d"
                             % (self.recipe.N, self.bank.min_rows))


def bank_arrays(arrays: Sequence, what: str):
    """The bank's arrays as float32 [rows, row_len]: one row length, none empty (`what` one of them is called)."""
    arrays = [np.asarray(a, dtype=np.float32) for a in arrays]
    if not arrays or any(a.ndim != 2 or a.shape[1] != arrays[0].shape[1] for a in arrays):
        raise ValueError("build_cpu: %ss are [rows, row_len] arrays of one row length" % what)
    if any(a.shape[0] == 0 for a in arrays):
        raise ValueError("build_cpu: an empty %s" % what)
    return arrays


def host_twin(spec: ops.CloudBatchSpec, c_struct, arrays: Sequence[np.ndarray], what: str, ids, count: Optional[int],
              bank: Optional[dict] = None, counter: tuple = (0, 0), draws: Optional[Dict[str, np.ndarray]] = None,
              num_threads: Optional[int] = None):
    """What the four build_cpu share, and the call of usip_<tag>_build_f32_cpu.  arrays: the bank's [rows, row_len] arrays
    (`what` one of them is called); c_struct: row_len -> the recipe struct; count: the ids a call must have (None: any);
    bank: what the bank struct holds beside rows, offsets and min_rows; counter: (seed, step[, pair_base]); draws: arrays
    in the header's layouts, or None for Philox draws.  Returns (outputs, rows, node_slots) as numpy arrays."""
    arrays = bank_arrays(arrays, what)
    recipe = c_struct(arrays[0].shape[1])
    c = ops.cloud_recipe(recipe)
    lengths = [len(a) for a in arrays]
    bank = dict(bank or {}, rows=np.ascontiguousarray(np.concatenate(arrays)), min_rows=min(lengths),
                offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
    n = ids.size
    if count is not None and n != int(count):
        raise ValueError("build_cpu: %d %s ids for %d pairs" % (n, spec.ids, count))
    out = {k: np.zeros(shape, dtype=_NP[dt]) for k, (shape, dt) in ops.cloud_batch_table(spec, recipe, n).items()}
    rows = np.zeros(spec.index_lead(n) + (c.N,), dtype=np.int32)
    nodes = np.zeros(spec.index_lead(n) + (c.M,), dtype=np.int32)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = None
    if draws is not None:
        draws = {k: np.ascontiguousarray(draws[k], dtype=_NP[dt]) for k, dt in spec.draws.items()
                 if draws.get(k) is not None}
        ops.check_draws(spec, c, n, draws, ValueError)
        d = ops.draws_struct(spec, ptr, draws)
    b = ops.bank_struct(spec, ptr, bank)
    o = ops.out_struct(spec, ptr, out, rows, nodes)
    symbol = "usip_%s_build_f32_cpu" % spec.tag
    args = (ctypes.addressof(recipe), ctypes.addressof(d) if d is not None else None)
    args += spec.lead(ptr, bank, b, ptr(ids), n, None, False) + ops.counter_args(counter) + (ctypes.addressof(o),)
    _lib.check(getattr(_lib.lib(), symbol)(*args, *(() if num_threads is None else (int(num_threads),))), symbol)
    return out, rows, nodes


def build_cpu(recipe: PairRecipe, scans: Sequence[np.ndarray], scan_ids, pairs: int, seed: int = 0, step: int = 0,
              rank: int = 0, mode: str = "train", draws: Optional[Dict[str, np.ndarray]] = None):
    """The host twin (usip_pairs_build_f32_cpu) on numpy scans: Philox draws, or `draws` (the layouts of
    include/usip_hip.h).  Returns (batch, rows [2,P,N], node_slots [2,P,M])."""
    return host_twin(ops.PAIRS, lambda row_len: recipe.c_struct(mode == "train"), scans, "scan", scan_ids, pairs,
                     counter=(seed, step, rank * int(pairs)), draws=draws)


