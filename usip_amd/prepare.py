"""Raw LiDAR scans prepared on the device: raw scan in, the reference's [rows, 8] scan out.

The reference prepares its scans with MATLAB (evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108):
findPointNormals(pc, 9, [0, 0, 1], true) -- nine nearest neighbours through a kd-tree, a 3x3 covariance about the point, its
smallest eigenvector, a flip towards a view point -- then pcdownsample(pc, 'gridAverage', 0.2).  Here the same three stages
run as HIP kernels on a scan that is already in device memory (csrc/prepare.hip; the semantics are restated in
include/usip_hip.h and csrc/prepare_math.h):

    prep = ScanPreparer("cuda:0", k=9, leaf=0.2, viewpoint=(0., 0., 1.))
    rows = prep(load_velodyne_bin("000000.bin"))        # f32 [n,4] -> f32 device tensor [m,8]
    bank = pairs.ScanBank.from_device_rows([rows, ...])  # ... and straight into the training-pair builder

  ScanPreparer.normals   per-point (nx ny nz curvature) in float64 and the neighbour indices
  prepare_cpu            the same on numpy arrays over the library's host twins (csrc/prepare_cpu.cpp)
  load_velodyne_bin / save_test_bin   a KITTI .bin in; [m,6] xyz + normal out, as kitti_test_prepare.m writes

Sorting (the points along x for the neighbour search, the cell keys for the grid) and the segment starts are torch
plumbing; the grid stage reads the number of occupied cells back, the one host synchronisation of a call.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops


def _frame(frame) -> Optional[np.ndarray]:
    if frame is None:
        return None
    f = np.asarray(frame, dtype=np.float64)
    if f.shape != (3, 4):
        raise ValueError("frame must be 3x4 (rotation | translation), got %s" % (f.shape,))
    return f


def _keep_rows(m: int, max_rows: Optional[int], seed: int, scan_id: int) -> Optional[torch.Tensor]:
    """The rows kept when m > max_rows: max_rows of them, chosen by a CPU generator seeded from (seed, scan_id), ascending."""
    if max_rows is None or m <= int(max_rows):
        return None
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 1000003 + int(scan_id)) & 0x7FFFFFFFFFFFFFFF)
    return torch.sort(torch.randperm(m, generator=g)[:int(max_rows)]).values


def _finish(rows: torch.Tensor, frame: Optional[np.ndarray], keep: Optional[torch.Tensor]) -> torch.Tensor:
    """frame applied to xyz and its rotation to the normal (float64, then rounded once), then the kept rows."""
    if frame is not None:
        f = torch.from_numpy(frame).to(rows.device)
        R, t = f[:, :3], f[:, 3]
        out = rows.clone()
        out[:, 0:3] = (rows[:, 0:3].double() @ R.T + t).float()
        out[:, 3:6] = (rows[:, 3:6].double() @ R.T).float()
        rows = out
    if keep is not None:
        rows = rows[keep.to(rows.device)].contiguous()
    return rows


class ScanPreparer:
    """One raw scan per call: xyzi [n,4] (numpy or tensor; x y z reflectance) -> float32 device tensor [m,8]
    (x y z nx ny nz curvature reflectance), voxel-averaged at `leaf`, rows in ascending cell-key order.

    frame: a rigid 3x4 (e.g. KITTI's velodyne -> camera Tr) applied to the prepared rows; max_rows (the reference's 20480):
    when more cells are occupied, max_rows of them are kept, drawn from (seed, scan_id), in ascending row order."""

    def __init__(self, device="cuda:0", k: int = 9, leaf: float = 0.2, viewpoint: Sequence[float] = (0.0, 0.0, 1.0),
                 frame=None, max_rows: Optional[int] = None, seed: int = 0):
        self.device = torch.device(device)
        self.k, self.leaf = int(k), float(leaf)
        self.viewpoint = tuple(float(v) for v in viewpoint)
        if not 1 <= self.k <= 16 or not self.leaf > 0.0 or len(self.viewpoint) != 3:
            raise ValueError("ScanPreparer: k in 1..16, leaf > 0, viewpoint of three numbers")
        self.frame, self.max_rows, self.seed = _frame(frame), max_rows, int(seed)

    def _scan(self, xyzi) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(xyzi, dtype=np.float32)) if isinstance(xyzi, np.ndarray) else xyzi
        if t.dim() != 2 or t.shape[1] != 4:
            raise ValueError("a raw scan must be [n,4] (x y z reflectance), got %s" % (tuple(t.shape),))
        return t.to(self.device, torch.float32).contiguous()

    def neighbours(self, xyzi, want_visits: bool = False):
        """idx i32 [n,K]; want_visits: also the tiles each workgroup walked (the share of the n^2 pairs visited)."""
        pts = self._scan(xyzi)
        perm = torch.sort(pts[:, 0], stable=True).indices.to(torch.int32)
        return ops.scan_knn(pts, perm, self.k, want_visits)

    def normals(self, xyzi) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (f64 [n,4] nx ny nz curvature, idx i32 [n,K])"""
        pts = self._scan(xyzi)
        idx = self.neighbours(pts)
        return ops.scan_normals(pts, idx, self.viewpoint)[0], idx

    def grid(self, pts: torch.Tensor, nrm64: torch.Tensor):
        """-> (rows f32 [m,8], keys i64 [m], perm i32 [n], start i32 [m+1]) of the voxel grid average"""
        lo, hi = torch.aminmax(pts[:, :3], dim=0)
        keys = ops.scan_voxel_keys(pts, torch.cat((lo, hi)).contiguous(), self.leaf)
        skeys, order = torch.sort(keys, stable=True)
        cells, counts = torch.unique_consecutive(skeys, return_counts=True)
        start = torch.zeros(cells.shape[0] + 1, dtype=torch.int32, device=pts.device)   # (the one host read: m)
        start[1:] = torch.cumsum(counts, 0)
        rows = ops.scan_voxel_average(pts, nrm64, order.to(torch.int32), start)
        return rows, cells, order.to(torch.int32), start

    def __call__(self, xyzi, scan_id: int = 0) -> torch.Tensor:
        pts = self._scan(xyzi)
        with torch.cuda.device(self.device):
            nrm64, _ = self.normals(pts)
            rows = self.grid(pts, nrm64)[0]
            return _finish(rows, self.frame, _keep_rows(rows.shape[0], self.max_rows, self.seed, scan_id))


# ------------------------------------------------------------------------------------------------ host twins (numpy)
def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _scan_np(xyzi) -> np.ndarray:
    a = np.ascontiguousarray(xyzi, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("a raw scan must be [n,4] (x y z reflectance), got %s" % (a.shape,))
    return a


def knn_cpu(xyzi, k: int = 9, num_threads: int = 1) -> np.ndarray:
    a = _scan_np(xyzi)
    idx = np.zeros((a.shape[0], int(k)), np.int32)
    _lib.check(_lib.lib().usip_scan_knn_f32_cpu(_p(a), a.shape[0], int(k), _p(idx), int(num_threads)),
               "usip_scan_knn_f32_cpu")
    return idx


def normals_cpu(xyzi, idx=None, k: int = 9, viewpoint=(0.0, 0.0, 1.0), num_threads: int = 1):
    """-> (f64 [n,4] nx ny nz curvature, idx i32 [n,K], f32 [n,4])"""
    a = _scan_np(xyzi)
    idx = knn_cpu(a, k, num_threads) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    n, K = idx.shape
    view = np.asarray(viewpoint, dtype=np.float64).reshape(3).copy()
    n64, n32 = np.zeros((n, 4), np.float64), np.zeros((n, 4), np.float32)
    _lib.check(_lib.lib().usip_scan_normals_f32_cpu(_p(a), _p(idx), a.shape[0], K, _p(view), _p(n64), _p(n32)),
               "usip_scan_normals_f32_cpu")
    return n64, idx, n32


def grid_cpu(xyzi, nrm64, leaf: float = 0.2):
    """-> (rows f32 [m,8], keys i64 [m], perm i32 [n], start i32 [m+1])"""
    a = _scan_np(xyzi)
    n = a.shape[0]
    nrm64 = np.ascontiguousarray(nrm64, dtype=np.float64)
    if nrm64.shape != (n, 4):
        raise ValueError("normals must be f64 [n,4]")
    lohi = np.concatenate((a[:, :3].min(0), a[:, :3].max(0))).astype(np.float32)
    keys = np.zeros(n, np.int64)
    _lib.check(_lib.lib().usip_scan_voxel_keys_f32_cpu(_p(a), n, _p(lohi), float(leaf), _p(keys)),
               "usip_scan_voxel_keys_f32_cpu")
    order = np.argsort(keys, kind="stable").astype(np.int32)
    cells, first = np.unique(keys[order], return_index=True)
    start = np.concatenate((first, [n])).astype(np.int32)
    rows = np.zeros((cells.shape[0], 8), np.float32)
    _lib.check(_lib.lib().usip_scan_voxel_average_f32_cpu(_p(a), _p(nrm64), _p(order), _p(start), n, cells.shape[0],
                                                          _p(rows)), "usip_scan_voxel_average_f32_cpu")
    return rows, cells, order, start


def prepare_cpu(xyzi, k: int = 9, leaf: float = 0.2, viewpoint=(0.0, 0.0, 1.0), frame=None, max_rows: Optional[int] = None,
                seed: int = 0, scan_id: int = 0, num_threads: int = 1) -> np.ndarray:
    """ScanPreparer.__call__ on the host: -> f32 [m,8]."""
    a = _scan_np(xyzi)
    nrm64, _, _ = normals_cpu(a, None, k, viewpoint, num_threads)
    rows = torch.from_numpy(grid_cpu(a, nrm64, leaf)[0])
    return _finish(rows, _frame(frame), _keep_rows(rows.shape[0], max_rows, seed, scan_id)).numpy()


# ------------------------------------------------------------------------------------------------ files
def load_velodyne_bin(path) -> np.ndarray:
    """A KITTI velodyne .bin: float32 [n,4] x y z reflectance."""
    a = np.fromfile(path, dtype=np.float32)
    if a.size % 4:
        raise ValueError("%s: %d float32 values are not rows of 4" % (path, a.size))
    return a.reshape(-1, 4)


def save_test_bin(path, rows) -> None:
    """xyz + normal, float32 [m,6], as kitti_test_prepare.m writes its test scans."""
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    if a.ndim != 2 or a.shape[1] < 6:
        raise ValueError("rows must be [m,8] (or [m,6])")
    np.ascontiguousarray(a[:, :6], dtype=np.float32).tofile(path)
