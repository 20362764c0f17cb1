"""Tensor-level wrappers over the C ABI (include/usip_hip.h).

Every function takes contiguous device tensors, allocates its outputs with torch (device
memory + stream plumbing only), enqueues the HIP kernels on torch's CURRENT stream and
returns without synchronising.  Host tensors raise RuntimeError: there is no CPU path here.
"""
import ctypes
import functools
import math
import os
import types
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib, prof


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need(t: torch.Tensor, name: str, dtype):
    # mirrors CHECK_INPUT of the reference (index_max.cpp:119-121, ball_query.cpp:10-12):
    # device + contiguous, reported as RuntimeError; dtype is checked too (the reference
    # would read garbage).
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor/variable" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))


def _ptr(t: torch.Tensor):
    return ctypes.c_void_p(t.data_ptr())


def index_max(data: torch.Tensor, index: torch.Tensor, K: int) -> torch.Tensor:
    """a-1: data f32 [B,C,N], index i32 [B,N] -> i32 [B,C,K] (index_max_cuda.cu:83-98)."""
    K = int(K)
    _need(data, "data", torch.float32)
    _need(index, "index", torch.int32)
    if data.dim() != 3 or index.dim() != 2 or index.shape[0] != data.shape[0] or index.shape[1] != data.shape[2]:
        raise RuntimeError("index_max: expected data [B,C,N] and index [B,N]")
    B, C, N = data.shape
    out = torch.empty((B, C, int(K)), dtype=torch.int32, device=data.device)
    with torch.cuda.device(data.device), prof.kernel("index_max", 4.0 * (B * C * N + B * N + B * C * K)):
        _lib.check(_lib.lib().usip_index_max_f32(_ptr(data), _ptr(index), _ptr(out), B, C, N, int(K),
                                                 _stream(data)), "usip_index_max_f32")
    return out


def index_max_values(data: torch.Tensor, index: torch.Tensor, count, K: int, C: Optional[int] = None):
    """index_max plus the gather + mask the reference applies to it (networks.py:117-118): -> (max_idx i32 [B,C,K],
    data[b,c,max_idx] * (count > 0) f32 [B,C,K]).  data [B,Ctot,N]; C: use only the first C channels.
    The values equal gather * mask numerically; a winning -0.0 is returned as +0.0 (csrc/index_max.hip: the two zeros tie
    in the key).  count None: every node counts.  index must lie in [0, K): the kernel does not guard it."""
    K = int(K)
    _need(data, "data", torch.float32)
    _need(index, "index", torch.int32)
    if data.dim() != 3 or index.dim() != 2 or index.shape[0] != data.shape[0] or index.shape[1] != data.shape[2]:
        raise RuntimeError("index_max_values: expected data [B,C,N] and index [B,N]")
    B, Ctot, N = data.shape
    C = Ctot if C is None else int(C)
    if count is not None:
        _need(count, "count", torch.int32)
        if tuple(count.shape) != (B, K):
            raise RuntimeError("index_max_values: count must be [B,K]")
    idx = torch.empty((B, C, K), dtype=torch.int32, device=data.device)
    val = torch.empty((B, C, K), dtype=torch.float32, device=data.device)
    with torch.cuda.device(data.device), prof.kernel("index_max", 4.0 * (B * C * N + B * N + 2 * B * C * K)):
        _lib.check(_lib.lib().usip_index_max_values_f32(_ptr(data), _ptr(index), _opt(count), _ptr(idx), _ptr(val),
                                                        B, C, Ctot, N, K, _stream(data)), "usip_index_max_values_f32")
    return idx, val


def index_max_values_backward_add_(ddata, g, max_idx, count, coff: int = 0):
    """ddata[b, coff+c, max_idx[b,c,k]] += g[b,c,k] (populated nodes), in place; ddata [B,Ctot,N]."""
    _need(ddata, "ddata", torch.float32)
    _need(g, "g", torch.float32)
    B, Ctot, N = ddata.shape
    _, C, K = g.shape
    with torch.cuda.device(g.device), prof.kernel("index_max_bwd", 16.0 * B * C * K):
        _lib.check(_lib.lib().usip_index_max_values_backward_add_f32(_ptr(g), _ptr(max_idx), _opt(count), _ptr(ddata),
                                                                     B, C, Ctot, int(coff), N, K, _stream(g)),
                   "usip_index_max_values_backward_add_f32")
    return ddata


def index_max_values_backward(g, max_idx, count, index, N: int, src=None, soff: int = 0):
    """dz [B,C,N] = (src[:, soff:soff+C] if src is given else 0) + scatter of g [B,C,K] to max_idx (populated nodes):
    the gradient of index_max_values' masked values as one dense pass."""
    _need(g, "g", torch.float32)
    B, C, K = g.shape
    dz = torch.empty((B, C, int(N)), dtype=torch.float32, device=g.device)
    if src is not None:
        _need(src, "src", torch.float32)
    with torch.cuda.device(g.device), prof.kernel("index_max_bwd", 4.0 * B * C * N * (2 if src is not None else 1) + 4.0 * B * N):
        _lib.check(_lib.lib().usip_index_max_values_backward_f32(_ptr(g), _ptr(max_idx), _opt(count), _ptr(index),
                                                                 _opt(src), src.shape[1] if src is not None else 0,
                                                                 int(soff), _ptr(dz), B, C, int(N), K, _stream(g)),
                   "usip_index_max_values_backward_f32")
    return dz


def csr_by_index(idx32: torch.Tensor, N: int):
    """idx i32 [B,P] (values in [0,N)) -> (start i32 [B,N+1], perm i32 [B,P]): the positions sorted by destination."""
    _need(idx32, "idx", torch.int32)
    B, P = idx32.shape
    start = torch.empty((B, int(N) + 1), dtype=torch.int32, device=idx32.device)
    perm = torch.empty((B, P), dtype=torch.int32, device=idx32.device)
    with torch.cuda.device(idx32.device), prof.kernel("csr_by_index", 12.0 * B * P):
        _lib.check(_lib.lib().usip_csr_by_index_i32(_ptr(idx32), _ptr(start), _ptr(perm), B, P, int(N),
                                                    _stream(idx32)), "usip_csr_by_index_i32")
    return start, perm


def segment_sum_supported(N: int, P: int) -> bool:
    return bool(_lib.lib().usip_segment_sum_supported(int(N), int(P))) and int(N) <= 1820


def segment_sum(src, start, perm, C: int, coff: int = 0):
    """dx[b,c,n] = sum over segment n of src[b, coff+c, perm[b,j]]; src [B,Ctot,P] (any trailing shape) -> [B,C,N]."""
    _need(src, "src", torch.float32)
    B, Ctot = src.shape[0], src.shape[1]
    P = perm.shape[1]
    N = start.shape[1] - 1
    dx = torch.empty((B, int(C), N), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device), prof.kernel("segment_sum", 4.0 * B * (C * (P + N) + P)):
        _lib.check(_lib.lib().usip_segment_sum_f32(_ptr(src), _ptr(start), _ptr(perm), _ptr(dx), B, int(C), N, P,
                                                   Ctot, int(coff), _stream(src)), "usip_segment_sum_f32")
    return dx


def index_max_geometry(B: int, C: int, N: int, K: int):
    """(channel rows per workgroup, prefetch depth, threads) usip_index_max_f32 picks for this shape
    (usip_index_max_geometry, csrc/index_max.hip); lets a profiler name the launch."""
    ch, u, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().usip_index_max_geometry(int(B), int(C), int(N), int(K), ctypes.byref(ch), ctypes.byref(u),
                                                  ctypes.byref(t)), "usip_index_max_geometry")
    return ch.value, u.value, t.value


def ball_query(dist: torch.Tensor, radius: float, K: int) -> torch.Tensor:
    """a-2: dist f32 [B,M,N] -> i32 [B,M,K] (ball_query_cuda.cu:53-70)."""
    K = int(K)
    _need(dist, "node_to_point_dist", torch.float32)
    if dist.dim() != 3:
        raise RuntimeError("ball_query: expected dist [B,M,N]")
    B, M, N = dist.shape
    out = torch.empty((B, M, int(K)), dtype=torch.int32, device=dist.device)
    with torch.cuda.device(dist.device), prof.kernel("ball_query", 4.0 * (B * M * N + B * M * K)):
        _lib.check(_lib.lib().usip_ball_query_f32(_ptr(dist), _ptr(out), float(radius), int(K), B, M, N,
                                                  _stream(dist)), "usip_ball_query_f32")
    return out


def pairwise_dist(a: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """|a[b,:,m] - x[b,:,n]| -> f32 [B,M,N]; a [B,3,M], x [B,3,N]."""
    _need(a, "a", torch.float32)
    _need(x, "x", torch.float32)
    if a.dim() != 3 or x.dim() != 3 or a.shape[1] != 3 or x.shape[1] != 3 or a.shape[0] != x.shape[0]:
        raise RuntimeError("pairwise_dist: expected a [B,3,M], x [B,3,N]")
    B, _, M = a.shape
    N = x.shape[2]
    out = torch.empty((B, M, N), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device), prof.kernel("pairwise_dist", 4.0 * (B * M * N + 3 * B * (M + N))):
        _lib.check(_lib.lib().usip_pairwise_dist_f32(_ptr(a), _ptr(x), _ptr(out), B, M, N, _stream(a)),
                   "usip_pairwise_dist_f32")
    return out


def ball_query_coords(node: torch.Tensor, x: torch.Tensor, radius: float, K: int) -> torch.Tensor:
    """f-2: fused pairwise_dist + ball_query; node [B,3,M], x [B,3,N] -> i32 [B,M,K]."""
    K = int(K)
    _need(node, "node", torch.float32)
    _need(x, "x", torch.float32)
    if node.dim() != 3 or x.dim() != 3 or node.shape[1] != 3 or x.shape[1] != 3 or node.shape[0] != x.shape[0]:
        raise RuntimeError("ball_query_coords: expected node [B,3,M], x [B,3,N]")
    B, _, M = node.shape
    N = x.shape[2]
    out = torch.empty((B, M, int(K)), dtype=torch.int32, device=node.device)
    with torch.cuda.device(node.device), prof.kernel("ball_query_coords", 4.0 * (3 * B * (M + N) + B * M * K),
                                                    8.0 * B * M * N):
        _lib.check(_lib.lib().usip_ball_query_coords_f32(_ptr(node), _ptr(x), _ptr(out), float(radius), int(K),
                                                         B, M, N, _stream(node)), "usip_ball_query_coords_f32")
    return out


def _need_pts(t, name):
    _need(t, name, torch.float32)
    if t.dim() != 3 or t.shape[1] != 3:
        raise RuntimeError("%s must be [B,3,N]" % name)


def som_assign(x: torch.Tensor, node: torch.Tensor) -> torch.Tensor:
    """a-3: nearest SOM node of every point. x [B,3,N], node [B,3,M] -> min_idx i32 [B,N]."""
    _need_pts(x, "x")
    _need_pts(node, "node")
    B, _, N = x.shape
    M = node.shape[2]
    out = torch.empty((B, N), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device), prof.kernel("som_assign", 4.0 * (3 * B * (M + N) + B * N), 9.0 * B * M * N):
        _lib.check(_lib.lib().usip_som_assign_f32(_ptr(x), _ptr(node), _ptr(out), B, N, M, _stream(x)),
                   "usip_som_assign_f32")
    return out


def som_cluster(x: torch.Tensor, min_idx: torch.Tensor, M: int, decenter: bool = True, csr=None):
    """a-4: (cluster_mean f32 [B,3,M], count i32 [B,M], x_decentered f32 [B,3,N] or None).  csr = (start, perm) of
    min_idx from csr_by_index: the cluster sums walk the sorted segments instead of scanning all assignments."""
    _need_pts(x, "x")
    _need(min_idx, "min_idx", torch.int32)
    B, _, N = x.shape
    if tuple(min_idx.shape) != (B, N):
        raise RuntimeError("som_cluster: min_idx must be [B,N] = %s (got %s)" % ((B, N), tuple(min_idx.shape)))
    mean = torch.empty((B, 3, int(M)), dtype=torch.float32, device=x.device)
    count = torch.empty((B, int(M)), dtype=torch.int32, device=x.device)
    dec = torch.empty_like(x) if decenter else None
    if csr is not None:
        with torch.cuda.device(x.device), prof.kernel("som_cluster", 4.0 * (8 * B * N + 5 * B * M)):
            _lib.check(_lib.lib().usip_som_cluster_csr_f32(_ptr(x), _ptr(min_idx), _ptr(csr[0]), _ptr(csr[1]), _ptr(mean),
                                                           _ptr(count), _ptr(dec) if decenter else None, B, N, int(M),
                                                           _stream(x)), "usip_som_cluster_csr_f32")
        return mean, count, dec
    with torch.cuda.device(x.device), prof.kernel("som_cluster", 4.0 * (7 * B * N + 4 * B * M)):
        _lib.check(_lib.lib().usip_som_cluster_f32(_ptr(x), _ptr(min_idx), _ptr(mean), _ptr(count),
                                                   _ptr(dec) if decenter else None, B, N, int(M), _stream(x)),
                   "usip_som_cluster_f32")
    return mean, count, dec


def nearest(a: torch.Tensor, b: torch.Tensor):
    """a-9/a-10 core: (min_j |a_i - b_j| f32 [B,Ma], first arg-min i32 [B,Ma])."""
    _need_pts(a, "a")
    _need_pts(b, "b")
    B, _, Ma = a.shape
    Nb = b.shape[2]
    d = torch.empty((B, Ma), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, Ma), dtype=torch.int32, device=a.device)
    ws = int(_lib.lib().usip_nearest_workspace(B, Ma, Nb))
    ws_d = torch.empty(ws, dtype=torch.float32, device=a.device) if ws else None
    ws_j = torch.empty(ws, dtype=torch.int32, device=a.device) if ws else None
    with torch.cuda.device(a.device), prof.kernel("nearest", 4.0 * (3 * B * (Ma + Nb) + 2 * B * Ma), 8.0 * B * Ma * Nb):
        _lib.check(_lib.lib().usip_nearest_f32(_ptr(a), _ptr(b), _ptr(d), _ptr(arg), _opt(ws_d), _opt(ws_j),
                                               B, Ma, Nb, _stream(a)), "usip_nearest_f32")
    return d, arg


# USIP_CELL_GRID=0: the Ball detector's ball query and the step's keypoint-on-cloud distances go back to the two
# brute-force launches (ball_query_coords, nearest) -- the A/B switch of csrc/cell_grid.hip; results are the same bits.
CELL_GRID = os.environ.get("USIP_CELL_GRID", "1") not in ("0", "off")


def cell_edge_factor() -> float:
    """Cell edge to ask cell_grid_build for = ball radius * this (usip_cell_grid_edge_factor, csrc/cell_grid.h)."""
    return float(_lib.lib().usip_cell_grid_edge_factor())


@functools.lru_cache(maxsize=None)
def _cell_hdr_word(name: str) -> int:
    w = int(_lib.lib().usip_cell_grid_hdr_word(name.encode()))
    if w < 0:
        raise RuntimeError("usip_amd: usip_cell_grid_hdr_word does not know %r" % name)
    return w



class CellGrid:
    """A cloud batch sorted into cells by cell_grid_build: x f32 [B,3,N] itself (the searches fall back to scanning it)
    and the three tensors of usip_cell_grid_build_f32.  header() reads the per-cloud header back (synchronises)."""

    def __init__(self, x, edge, hdr, cell_start, pts):
        self.x, self.edge, self.hdr, self.cell_start, self.pts = x, float(edge), hdr, cell_start, pts

    def built_from(self, x: torch.Tensor) -> bool:
        return x.data_ptr() == self.x.data_ptr() and x.shape == self.x.shape and x.is_contiguous()

    def header(self):
        h = self.hdr.cpu()
        f = h.view(torch.float32)
        w = _cell_hdr_word
        return [dict(origin=[float(f[b, w(k)]) for k in ("ox", "oy", "oz")], edge=float(f[b, w("edge")]),
                     inv=float(f[b, w("inv")]), dim=[int(h[b, w(k)]) for k in ("nx", "ny", "nz")],
                     usable=bool(h[b, w("usable")])) for b in range(h.shape[0])]


def cell_grid_build(x: torch.Tensor, edge: float, max_block: int = 0) -> CellGrid:
    """x [B,3,N] -> its CellGrid with cells at least `edge` wide (wider when the cloud needs more cells than the
    kernel counts).  max_block > 0: a cloud whose 27-cell blocks hold more points than that on average is dense, is
    left unsorted and its rows scan; ball_block_limit(N, K) for a grid that serves a ball query."""
    _need_pts(x, "x")
    B, _, N = x.shape
    cap = int(_lib.lib().usip_cell_grid_cap())
    hdr = torch.empty((B, _cell_hdr_word("words")), dtype=torch.int32, device=x.device)
    cell_start = torch.empty((B, cap + 1), dtype=torch.int32, device=x.device)
    pts = torch.empty((B, N, 4), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), prof.kernel("cell_grid_build", 4.0 * (3 * 3 * B * N + 4 * B * N), 0.0):
        _lib.check(_lib.lib().usip_cell_grid_build_f32(_ptr(x), float(edge), int(max_block), _ptr(hdr), _ptr(cell_start), _ptr(pts),
                                                       B, N, _stream(x)), "usip_cell_grid_build_f32")
    return CellGrid(x, edge, hdr, cell_start, pts)


def ball_block_limit(N: int, K: int) -> int:
    """cell_grid_build's max_block for a ball query with K samples: floor(sqrt(N * K)), the candidate count up to which a
    row of ball_query_grid_kernel takes the grid (cand^2 <= N * K).  From shapes alone."""
    return max(1, math.isqrt(int(N) * int(K)))


def ball_query_grid(node: torch.Tensor, grid: CellGrid, radius: float, K: int, with_route: bool = False):
    """ball_query_coords(node, grid.x, radius, K), bit for bit, through the grid; with_route: -> (idx, u8 [B,M] with 1
    where the row came from the grid and 0 where the launch scanned it in index order)."""
    K = int(K)
    _need(node, "node", torch.float32)
    x = grid.x
    if node.dim() != 3 or node.shape[1] != 3 or node.shape[0] != x.shape[0]:
        raise RuntimeError("ball_query_grid: expected node [B,3,M] for a grid of x [B,3,N]")
    B, _, M = node.shape
    N = x.shape[2]
    out = torch.empty((B, M, K), dtype=torch.int32, device=node.device)
    route = torch.empty((B, M), dtype=torch.uint8, device=node.device) if with_route else None
    # flops: the pair count of the brute-force launch this replaces (8 per pair, as "ball_query_coords"), NOT executed
    # work -- the grid tests a few dozen points per row; kept so that the two routes share a column in bench.py --full
    with torch.cuda.device(node.device), prof.kernel("ball_query_grid", 4.0 * (3 * B * M + B * M * K), 8.0 * B * M * N):
        _lib.check(_lib.lib().usip_ball_query_grid_f32(_ptr(node), _ptr(x), _ptr(grid.hdr), _ptr(grid.cell_start),
                                                       _ptr(grid.pts), _ptr(out), _opt(route), float(radius), K,
                                                       B, M, N, _stream(node)), "usip_ball_query_grid_f32")
    return (out, route) if with_route else out


def nearest_grid(a: torch.Tensor, grid: CellGrid, with_route: bool = False):
    """nearest(a, grid.x), bit for bit, through the grid; with_route as ball_query_grid."""
    _need_pts(a, "a")
    x = grid.x
    B, _, Ma = a.shape
    N = x.shape[2]
    if x.shape[0] != B or N < 1:
        raise RuntimeError("nearest_grid: expected a [B,3,Ma] for a grid of x [B,3,N], N >= 1")
    d = torch.empty((B, Ma), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, Ma), dtype=torch.int32, device=a.device)
    route = torch.empty((B, Ma), dtype=torch.uint8, device=a.device) if with_route else None
    # flops: the brute-force-equivalent pair count (8 per pair, as "nearest"), not executed work
    with torch.cuda.device(a.device), prof.kernel("nearest_grid", 4.0 * (3 * B * Ma + 2 * B * Ma), 8.0 * B * Ma * N):
        _lib.check(_lib.lib().usip_nearest_grid_f32(_ptr(a), _ptr(x), _ptr(grid.hdr), _ptr(grid.cell_start),
                                                    _ptr(grid.pts), _ptr(d), _ptr(arg), _opt(route), B, Ma, N,
                                                    _stream(a)), "usip_nearest_grid_f32")
    return (d, arg, route) if with_route else (d, arg)


def chamfer_prob(a, J, c, I, sigma_src, sigma_dst):
    """(loss, chamfer_pure, chamfer_weighted) as a 3-vector from the nearest-neighbour minima a [B,M] / J i32
    and c [B,N] / I i32 and the two sigma maps (models/losses.py:82-99)."""
    for t, n in ((a, "a"), (c, "c"), (sigma_src, "sigma_src"), (sigma_dst, "sigma_dst")):
        _need(t, n, torch.float32)
    _need(J, "J", torch.int32)
    _need(I, "I", torch.int32)
    B, M = a.shape
    N = c.shape[1]
    if J.shape != a.shape or I.shape != c.shape or sigma_src.shape != a.shape or sigma_dst.shape != c.shape:
        raise RuntimeError("chamfer_prob: shapes do not match")
    out = torch.empty(3, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device), prof.kernel("chamfer_prob", 4.0 * 3 * B * (M + N), 0.0):
        _lib.check(_lib.lib().usip_chamfer_prob_f32(_ptr(a), _ptr(J), _ptr(c), _ptr(I), _ptr(sigma_src),
                                                    _ptr(sigma_dst), _ptr(out), B, M, N, _stream(a)),
                   "usip_chamfer_prob_f32")
    return out


def chamfer_prob_backward(gloss, a, J, c, I, sigma_src, sigma_dst):
    """-> (da, dc, dsigma_src, dsigma_dst) for the upstream gradient `gloss` (0-dim device tensor) of the loss."""
    B, M = a.shape
    N = c.shape[1]
    _need(gloss, "gloss", torch.float32)
    da, dc = torch.empty_like(a), torch.empty_like(c)
    dss, dsd = torch.empty_like(sigma_src), torch.empty_like(sigma_dst)
    with torch.cuda.device(a.device), prof.kernel("chamfer_prob_bwd", 4.0 * 7 * B * (M + N), 0.0):
        _lib.check(_lib.lib().usip_chamfer_prob_backward_f32(_ptr(gloss), _ptr(a), _ptr(J), _ptr(c), _ptr(I),
                                                             _ptr(sigma_src), _ptr(sigma_dst), _ptr(da), _ptr(dc),
                                                             _ptr(dss), _ptr(dsd), B, M, N, _stream(a)),
                   "usip_chamfer_prob_backward_f32")
    return da, dc, dss, dsd


def bn_group_dy_sum(gsum, coef4, K: int):
    """sum over each neighbourhood's K positions of dY, [nb,C,G], from gsum = (sum dYhat, sum y) (each [nb,C,G])."""
    g0, g1 = gsum[0], gsum[1]
    nb, C, G = g0.shape
    out = torch.empty_like(g0)
    with torch.cuda.device(g0.device), prof.kernel("bn_group_dy_sum", 12.0 * g0.numel()):
        _lib.check(_lib.lib().usip_bn_group_dy_sum_f32(_ptr(g0), _ptr(g1), _ptr(coef4), _ptr(out), nb, C, G, int(K),
                                                       _stream(g0)), "usip_bn_group_dy_sum_f32")
    return out


def detector_head(ks, centre, sigma_lower_bound: float):
    """ks [B,4,M] (mlp3 output), centre [B,3,M] -> (keypoints [B,3,M], sigmas [B,M]) (networks.py:150-154)."""
    _need(ks, "ks", torch.float32)
    _need(centre, "centre", torch.float32)
    B, _, M = ks.shape
    kp = torch.empty((B, 3, M), dtype=torch.float32, device=ks.device)
    sg = torch.empty((B, M), dtype=torch.float32, device=ks.device)
    with torch.cuda.device(ks.device), prof.kernel("head", 4.0 * 11 * B * M):
        _lib.check(_lib.lib().usip_detector_head_f32(_ptr(ks), _ptr(centre), float(sigma_lower_bound), _ptr(kp), _ptr(sg),
                                                     B, M, _stream(ks)), "usip_detector_head_f32")
    return kp, sg


def detector_head_backward(g_kp, g_sg, ks):
    B, _, M = ks.shape
    g = torch.empty_like(ks)
    with torch.cuda.device(ks.device), prof.kernel("head_bwd", 4.0 * 9 * B * M):
        _lib.check(_lib.lib().usip_detector_head_backward_f32(_opt(g_kp), _opt(g_sg), _ptr(ks), _ptr(g), B, M,
                                                              _stream(ks)), "usip_detector_head_backward_f32")
    return g


def rigid_transform(x, R, scale, shift, transpose: bool = False):
    """(R*scale) . x + shift per cloud (keypoint_detector.py:182-184); transpose: (R*scale)^T . x (the backward)."""
    _need(x, "x", torch.float32)
    B, _, M = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device), prof.kernel("rigid_transform", 4.0 * 6 * B * M):
        _lib.check(_lib.lib().usip_rigid_transform_f32(_ptr(x), _ptr(R), _ptr(scale), _opt(shift), _ptr(out),
                                                       int(bool(transpose)), B, M, _stream(x)),
                   "usip_rigid_transform_f32")
    return out


def detector_loss_combine(d, chamfer, alpha: float):
    """d [2B,M] keypoint-to-cloud distances (src rows first), chamfer: 0-dim/1-element loss tensor ->
    3-vector (loss, alpha*mean(d_src), alpha*mean(d_dst)) (keypoint_detector.py:196-204)."""
    _need(d, "d", torch.float32)
    out = torch.empty(3, dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device), prof.kernel("loss_combine", 4.0 * d.numel()):
        _lib.check(_lib.lib().usip_detector_loss_combine_f32(_ptr(d), _ptr(chamfer), float(alpha), _ptr(out),
                                                             d.numel() // 2, _stream(d)),
                   "usip_detector_loss_combine_f32")
    return out


def fill_scaled(g, factor: float, shape):
    """A tensor of `shape` filled with g[0] * factor (g: device scalar)."""
    out = torch.empty(shape, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device), prof.kernel("fill_scaled", 4.0 * out.numel()):
        _lib.check(_lib.lib().usip_fill_scaled_f32(_ptr(g), float(factor), _ptr(out), out.numel(), _stream(g)),
                   "usip_fill_scaled_f32")
    return out


# USIP_LOSS_TAIL=0: the detector step's loss segment goes back to the chain of launches (rigid_transform, 2 x nearest,
# chamfer_prob, loss_combine and their backwards) -- the A/B switch of csrc/loss_tail.hip; results are the same bits.
LOSS_TAIL = os.environ.get("USIP_LOSS_TAIL", "1") not in ("0", "off")
LOSS_TAIL_MAX_M = 1024                                        # a pair's keypoints are staged in LDS


def loss_tail_scan(kp, R, scale, shift):
    """kp [2B,3,M] (src clouds first) -> (kp_t [B,3,M], a, J, c, I [B,M]): rigid_transform of the src half and nearest
    in both directions against the dst half, bit for bit, in one launch."""
    _need_pts(kp, "keypoints")
    for t, n in ((R, "R"), (scale, "scale"), (shift, "shift")):
        _need(t, n, torch.float32)
    B, M = kp.shape[0] // 2, kp.shape[2]
    if kp.shape[0] != 2 * B or R.numel() != 9 * B or scale.numel() != B or shift.numel() != 3 * B:
        raise RuntimeError("loss_tail_scan: expected keypoints [2B,3,M], R [B,3,3], scale [B], shift [B,3]")
    kp_t = torch.empty((B, 3, M), dtype=torch.float32, device=kp.device)
    a, c = (torch.empty((B, M), dtype=torch.float32, device=kp.device) for _ in range(2))
    J, I = (torch.empty((B, M), dtype=torch.int32, device=kp.device) for _ in range(2))
    with torch.cuda.device(kp.device), prof.kernel("loss_tail_scan", 4.0 * (9 * B * M + 4 * B * M), 2 * 8.0 * B * M * M):
        _lib.check(_lib.lib().usip_loss_tail_scan_f32(_ptr(kp), _ptr(R), _ptr(scale), _ptr(shift), _ptr(kp_t), _ptr(a),
                                                      _ptr(J), _ptr(c), _ptr(I), B, M, _stream(kp)),
                   "usip_loss_tail_scan_f32")
    return kp_t, a, J, c, I


def loss_tail_sums(a, J, c, I, sg, d, alpha: float):
    """-> 6-vector (loss, loss_chamfer, chamfer_pure, chamfer_weighted, alpha*mean(d_src), alpha*mean(d_dst)): chamfer_prob
    on (a, J, c, I) and the two halves of sg [2B,M], then detector_loss_combine on d [2B,M], in one launch."""
    for t, n in ((a, "a"), (c, "c"), (sg, "sigmas"), (d, "d")):
        _need(t, n, torch.float32)
    _need(J, "J", torch.int32)
    _need(I, "I", torch.int32)
    B, M = a.shape
    if not (J.shape == I.shape == c.shape == a.shape) or tuple(sg.shape) != (2 * B, M) or tuple(d.shape) != (2 * B, M):
        raise RuntimeError("loss_tail_sums: shapes do not match")
    out = torch.empty(6, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device), prof.kernel("loss_tail_sums", 4.0 * 8 * B * M, 0.0):
        _lib.check(_lib.lib().usip_loss_tail_sums_f32(_ptr(a), _ptr(J), _ptr(c), _ptr(I), _ptr(sg), _ptr(d), float(alpha),
                                                      _ptr(out), B, M, _stream(a)), "usip_loss_tail_sums_f32")
    return out


def loss_tail_backward(gloss, kp, sg, kp_t, a, J, c, I, d, arg, pc, R, scale, factor: float):
    """-> (g_kp [2B,3,M], g_sg [2B,M]) for the upstream gradient `gloss` (device scalar) of the loss; (d, arg) are the
    keypoint-to-cloud minima against pc [2B,3,N]; factor: what fill_scaled gets for d's gradient, alpha / (B * M)."""
    _need(gloss, "gloss", torch.float32)
    _need_pts(pc, "pc")
    _need(arg, "arg", torch.int32)
    B, M = a.shape
    if pc.shape[0] != 2 * B or tuple(d.shape) != (2 * B, M) or tuple(arg.shape) != (2 * B, M):
        raise RuntimeError("loss_tail_backward: shapes do not match")
    g_kp, g_sg = torch.empty_like(kp), torch.empty_like(sg)
    with torch.cuda.device(kp.device), prof.kernel("loss_tail_bwd", 4.0 * 30 * B * M, 0.0):
        _lib.check(_lib.lib().usip_loss_tail_backward_f32(_ptr(gloss), _ptr(kp), _ptr(sg), _ptr(kp_t), _ptr(a), _ptr(J),
                                                          _ptr(c), _ptr(I), _ptr(d), _ptr(arg), _ptr(pc), _ptr(R),
                                                          _ptr(scale), float(factor), _ptr(g_kp), _ptr(g_sg), B, M,
                                                          pc.shape[2], _stream(kp)), "usip_loss_tail_backward_f32")
    return g_kp, g_sg


# --------------------------------------------------------------------------- shared MLP
def _opt(t):
    return _ptr(t) if t is not None else None


# "f32": fp32 MFMA (the parity mode and the headline).  "bf16": operands rounded to bf16 inside the GEMM and
# weight-gradient kernels, fp32 accumulate, everything else fp32 (BASELINE.json configs[1] perf mode).
#   "f32x3": fp32-accurate products on the bf16 matrix cores (three bf16 planes per operand, six plane products) for
#   the matrix-bound launches, the fp32 kernel for the rest; results equal "f32" to fp32 rounding.
#   "f32x2": as f32x3, and the launches whose streamed operand has a rigorous bound (BatchNorm outputs forward, the
#   BatchNorm-backward operand with the bound usip_bn_backward_reduce_f32 computes) use TWO fp16 planes and THREE plane
#   products instead (half the matrix work, error at the same level); the others run the f32x3 kernel.
MATMUL_MODES = ("f32", "bf16", "f32x3", "f32x2")


def _x3_family() -> bool:
    return _matmul_mode in ("f32x3", "f32x2")
_matmul_mode = "f32"
import os as _os                                             # noqa: E402
if _os.environ.get("USIP_MATMUL_MODE"):                      # lets the whole GPU test suite run under another mode
    if _os.environ["USIP_MATMUL_MODE"] not in MATMUL_MODES:
        raise ValueError("USIP_MATMUL_MODE must be one of %s" % (MATMUL_MODES,))
    _matmul_mode = _os.environ["USIP_MATMUL_MODE"]


def set_matmul_mode(mode: str) -> str:
    """Select the multiply precision of the shared-MLP kernels; returns the previous mode."""
    global _matmul_mode
    if mode not in MATMUL_MODES:
        raise ValueError("matmul mode must be one of %s" % (MATMUL_MODES,))
    prev, _matmul_mode = _matmul_mode, mode
    return prev


def matmul_mode() -> str:
    return _matmul_mode


# f32x3 mode: split images of the weight operands (usip_mlp_split3_f32), keyed by (storage pointer, lda, column
# offset, M, K).  The training step sets this to a dict for the duration of one forward + backward (weights do not
# change in between), so every weight is split once per step; None: split at every call.
PLANES_CACHE = None


def weight_planes(At: torch.Tensor, a_offset: int, M: int, K: int, npl: int = 3, P: int = 0, nb: int = 1) -> torch.Tensor:
    """Split image (uint8 tensor) of the M x K operand A[m][k] = At[k, a_offset + m]: three bf16 planes for
    usip_mlp_gemm_x3p_f32 (npl 3) or two fp16 planes + scale for usip_mlp_gemm_x2h_f32 (npl 2), tiled for a launch over
    nb clouds of P positions (usip_mlp_x3p_tile_rows: small launches take 128-row tiles)."""
    lda = At.shape[1]
    rows = int(_lib.lib().usip_mlp_x3p_tile_rows(int(M), int(P), int(nb)))
    key = (At.data_ptr(), lda, int(a_offset), int(M), int(K), int(npl), rows)
    if PLANES_CACHE is not None and key in PLANES_CACHE:
        return PLANES_CACHE[key][1]
    nbytes = int(_lib.lib().usip_mlp_split3_bytes(M, K))
    planes = torch.empty(nbytes, dtype=torch.uint8, device=At.device)
    fn = "usip_mlp_split2h_f32" if npl == 2 else "usip_mlp_split3_f32"
    with torch.cuda.device(At.device), prof.kernel("weight_split3", 4.0 * M * K + nbytes):
        _lib.check(getattr(_lib.lib(), fn)(ctypes.c_void_p(At.data_ptr() + 4 * int(a_offset)), lda, M, K, rows,
                                           _ptr(planes), _stream(At)), fn)
    if PLANES_CACHE is not None:
        PLANES_CACHE[key] = (At, planes)      # holding At keeps its storage (the key) from being reused meanwhile
    return planes


class PlanesPlan:
    """The weight operands a step asks weight_planes() for, with persistent split images, refreshed by ONE launch at
    the start of the step (twelve 5-us launches otherwise).  Built from the PLANES_CACHE of a completed step; only
    operands inside the given persistent storages (parameters, their K-major copies) qualify -- their addresses are
    the cache keys, and a temporary's address could be handed out again."""

    def __init__(self, cache, storages):
        import numpy as np
        spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in storages if t is not None]
        self.entries, rows, blocks = {}, [], 0
        for key, (At, planes) in cache.items():
            ptr, lda, off, M, K, npl, trows = key
            if not any(lo <= ptr < hi for lo, hi in spans):
                continue
            self.entries[key] = (At, planes)
            rows.append((ptr + 4 * off, planes.data_ptr(), lda, M, K, blocks, trows, 2 if npl == 2 else 0))
            blocks += int(_lib.lib().usip_mlp_split3_blocks(M, K, trows))
        self.blocks = blocks
        dt = np.dtype(_lib.STRUCTS["usip_split3_desc"])      # the rows above are in the header's field order
        table = np.array(rows, dtype=dt) if rows else np.zeros(0, dtype=dt)
        dev = next(iter(self.entries.values()))[1].device if rows else None
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(dev) if rows else None

    def refresh(self):
        """Split every operand of the plan now; -> a PLANES_CACHE holding the fresh images."""
        if self.table is not None:
            with torch.cuda.device(self.table.device), prof.kernel("weight_split3", 0.0):
                _lib.check(_lib.lib().usip_mlp_split3_multi_f32(_ptr(self.table), len(self.entries), self.blocks,
                                                                _stream(self.table)), "usip_mlp_split3_multi_f32")
        return dict(self.entries)


# The narrow forward layers run the streaming kernel; USIP_NARROW_FWD=0 sends them through the generic tile kernel
# again (A/B measurement, tools/ab_env.sh).
NARROW_FWD = _os.environ.get("USIP_NARROW_FWD", "1") not in ("0", "off")
# The gradient of a layer output that is max-pooled AND passed on (functional.group_max_fork): the pooling part is added by
# the kernel that produces the dense part, at its store (csrc/gemm_x2f.hip: FORK), where that launch can;
# USIP_POOL_GRAD_FOLD=0 keeps the stand-alone pass (group_max_backward_add_) everywhere, for A/B runs.
POOL_GRAD_FOLD = _os.environ.get("USIP_POOL_GRAD_FOLD", "1") not in ("0", "off")


def mlp_gemm(At: torch.Tensor, X: torch.Tensor, bias=None, want_stats: bool = False, pro: int = 0,
             X2=None, coef=None, tag: str = "fwd", rowbias=None, rb_group: int = 1,
             M: Optional[int] = None, a_offset: int = 0, pool=None, a_trans: bool = False, out=None,
             out_row_offset: int = 0, red=None, red_group: int = 0, fork=None):
    """Y[b] = At^T . pro(X[b]) + bias (+ rowbias[b][:, p // rb_group]).
    At: K-major matrix operand, [K, lda] storage; the GEMM uses columns [a_offset, a_offset + M)
    (default: all of them).  X [nb,K,P] -> Y [nb,M,P] (+ stats [2,M,tiles] when want_stats).
    red = (y_prev [nb,M,P], coef_prev [>=4,M]) (data-gradient launches, pro 2 / 3): Y is the gradient of the lazily
    activated output of the layer with that pre-BN tensor and those coefficients; when the launch takes the direct f32x2
    kernel the call returns a THIRD value, the RedSums its epilogue left for that layer's BatchNorm backward (with .gsum
    [2,nb,M,P/red_group] when red_group is 16 or 32), else None as the third value.
    fork = (dpooled [nb,M,P/group], arg i32 [nb,M,P/group], group) (data-gradient launches, pro 2, without red): Y is the
    gradient of a tensor that is also max-pooled over runs of `group` positions; when the launch can
    (usip_mlp_gemm_x2h_fork_f32) the pooling gradient is added at its store -- Y then equals this launch followed by
    group_max_backward_add_ -- and the call returns True as a THIRD value, else it does nothing about it and returns False."""
    _need(At, "At", torch.float32)
    if a_trans:                               # At is [M_total, lda]: the operand is rows [m0, m0+M) x cols [a_offset, a_offset+K)
        M_rows, lda = At.shape
        M = M_rows if M is None else int(M)
        K = X2.shape[1] if X is None else X.shape[1]
    else:
        K, lda = At.shape
        M = lda if M is None else int(M)
    pool_dp = pool_arg = None
    pool_group = 0
    if pool is not None:                      # pro == 3: (dpooled [nb,K,G], arg i32 [nb,K,G], group); X unused
        pool_dp, pool_arg, pool_group = pool
        X = X2
    _need(X, "X", torch.float32)
    nb, Kx, P = X.shape
    if Kx != K or a_offset < 0 or a_offset + (K if a_trans else M) > lda:
        raise RuntimeError("mlp_gemm: operand shapes do not match (At %s, X %s, M %d, offset %d)"
                           % (tuple(At.shape), tuple(X.shape), M, a_offset))
    y_rows = 0
    if out is None:
        Y = torch.empty((nb, M, P), dtype=torch.float32, device=X.device)
        y_ptr = _ptr(Y)
    else:                                     # rows [out_row_offset, out_row_offset + M) of a wider [nb, rows, P] tensor
        _need(out, "out", torch.float32)
        if out.dim() != 3 or out.shape[0] != nb or out.shape[2] != P or out_row_offset < 0 \
                or out_row_offset + M > out.shape[1]:
            raise RuntimeError("mlp_gemm: out %s does not hold rows [%d, %d) of [%d, *, %d]"
                               % (tuple(out.shape), out_row_offset, out_row_offset + M, nb, P))
        Y, y_rows = out, out.shape[1]
        y_ptr = ctypes.c_void_p(out.data_ptr() + 4 * int(out_row_offset) * P)
    a_ptr = ctypes.c_void_p(At.data_ptr() + 4 * int(a_offset))
    # narrow layers (64 inputs, 64 / 128 outputs) at many positions: the streaming kernel (csrc/narrow_fwd.hip)
    # f32x2 mode: the 64 -> 128 layer (the feature half of conv4, with its row bias) goes to the register-resident f32x2
    # kernel -- the streaming kernel's fp32 MFMAs make it matrix-bound there (stand-alone 79-146 us depending on the box
    # against 82-109; in the step the same or better).
    lib = _lib.lib()
    rb_ok = rowbias is None or (rb_group % 32 == 0 and P % rb_group == 0)       # a row bias those two kernels can take
    x2r_direct = (_matmul_mode == "f32x2" and pro == 1 and coef is not None and coef.shape[0] >= 4
                  and M == 128 and K == 64 and not a_trans and pool is None and X2 is None and rb_ok
                  and nb * P >= 65536 and K * P < 2 ** 30)
    nf_blocks = 0
    if (NARROW_FWD and not x2r_direct and _matmul_mode != "bf16" and not a_trans and pool is None and X2 is None and pro in (0, 1)
            and K == 64 and M in (64, 128) and X.data_ptr() % 16 == 0 and rb_ok):
        nf_blocks = int(lib.usip_mlp_narrow_forward_blocks(M, K, P, nb))
    x3 = not nf_blocks and _x3_family() and (x2r_direct or bool(lib.usip_mlp_gemm_f32x3_used(M, K, P, nb)))
    x3p = x3 and not a_trans and K <= (512 if pro >= 2 else 640)       # weight operand split ahead of time
    # two fp16 planes: only where the streamed operand's bound is known (see usip_mlp_gemm_x2h_f32)
    x2h = (x3p and _matmul_mode == "f32x2" and coef is not None and
           ((pro == 1 and coef.shape[0] >= 4 and bound_covers(coef, nb * P)) or (pro >= 2 and coef.shape[0] >= 5)))
    # 128-wide layers: weight fragments resident in registers, persistent workgroups (usip_mlp_gemm_x2r_f32)
    x2r = (x2h and M <= 128 and K <= 128 and K * P < 2 ** 30                  # (usip_mlp_gemm_x2r_f32's own limits)
           and (rowbias is None or (pro == 1 and rb_ok and rb_group >= 32)))
    stats = None
    if want_stats:
        tiles = nf_blocks or (lib.usip_mlp_gemm_x2r_tiles(P, nb) if x2r else lib.usip_mlp_gemm_tiles(M, P, nb))
        stats = torch.empty((2, M, tiles), dtype=torch.float32, device=X.device)

    planes = weight_planes(At, a_offset, M, K, 2 if x2h else 3, P, nb) if x3p else None
    moved = 0.0
    if x3p:      # bytes into the CUs: per (tile, 16-k stage) the weight planes (L2) + the streamed operand, + the output
        bm_ = int(lib.usip_mlp_x3p_tile_rows(M, P, nb))
        bn_ = 128 if x2h else int(lib.usip_mlp_x3p_tile_cols(M, P, nb, int(pro), 1 if want_stats else 0))
        ntiles = nb * ((P + bn_ - 1) // bn_) * ((M + bm_ - 1) // bm_)
        moved = ntiles * ((K + 15) // 16) * ((2 if x2h else 3) * bm_ * 32 + 16 * bn_ * 4 * (2 if pro == 2 else 1)) \
            + 4.0 * nb * M * P
        if x2r:                                               # the weight fragments stay in registers
            moved = 4.0 * nb * P * (K * (2 if pro == 2 else 1) + M)
    plain_dgrad = x2h and not x2r and pro >= 2 and bias is None and rowbias is None     # what the red and fork launches take
    red_tiles = 0
    if (red is not None and plain_dgrad and out is None
            and red[1] is not None and red[1].shape[0] >= 4 and tuple(red[0].shape) == (nb, M, P)
            and red[0].is_contiguous() and red[0].data_ptr() % 16 == 0):
        red_tiles = int(lib.usip_mlp_gemm_x2d_red_tiles(M, K, P, nb, int(red_group)))
    fork_fold = False
    if fork is not None and plain_dgrad and pro == 2 and red is None and not want_stats and POOL_GRAD_FOLD:
        f_dp, f_arg, f_group = fork
        _need(f_dp, "fork dpooled", torch.float32)
        _need(f_arg, "fork arg", torch.int32)
        fork_fold = bool(f_group > 0 and P % f_group == 0 and tuple(f_dp.shape) == (nb, M, P // f_group)
                         and f_arg.shape == f_dp.shape and f_dp.data_ptr() % 16 == 0 and f_arg.data_ptr() % 16 == 0
                         and X.data_ptr() % 16 == 0 and X2.data_ptr() % 16 == 0 and y_ptr.value % 16 == 0
                         and lib.usip_mlp_gemm_x2h_fork_supported(M, K, P, nb, int(f_group)))
    third = None                                              # red: the RedSums or None; fork: folded or not
    x_ptr = None if pool is not None else _ptr(X)
    epi = (_opt(coef), int(pro), _opt(bias), _opt(rowbias), int(rb_group))
    pooled = (_opt(pool_dp), _opt(pool_arg), int(pool_group))
    shape = (M, K, P, nb, _stream(X))
    if nf_blocks:
        fn, args = "usip_mlp_narrow_forward_f32", (a_ptr, lda, x_ptr) + epi + (y_ptr, int(y_rows), _opt(stats))
    elif red_tiles:
        flat = torch.empty(2 * red_tiles * M + red_tiles * (M // 256), dtype=torch.float32, device=X.device)
        third = RedSums(flat, M, blocks=red_tiles)
        third.gsum = torch.empty((2, nb, M, P // red_group), dtype=torch.float32, device=X.device) if red_group else None
        fn, args = "usip_mlp_gemm_x2h_red_f32", (_ptr(planes), x_ptr, _opt(X2), _opt(coef), int(pro)) + pooled + (
            y_ptr, _ptr(red[0]), _ptr(red[1]), _ptr(flat), _opt(third.gsum), int(red_group))
    elif fork_fold:
        third = True
        fn, args = "usip_mlp_gemm_x2h_fork_f32", (_ptr(planes), _ptr(X), _ptr(X2), _ptr(coef), y_ptr, int(y_rows),
                                                  _ptr(f_dp), _ptr(f_arg), int(f_group))
    else:       # the entries that share usip_mlp_gemm_f32's signature, with the split image in place of (At, lda) for three
        fn = (("usip_mlp_gemm_x2r_f32" if x2r else "usip_mlp_gemm_x2h_f32" if x2h else "usip_mlp_gemm_x3p_f32") if x3p else
              {"bf16": "usip_mlp_gemm_bf16", "f32x3": "usip_mlp_gemm_f32x3", "f32x2": "usip_mlp_gemm_f32x3"}.get(
                  _matmul_mode, "usip_mlp_gemm_f32"))
        args = ((_ptr(planes),) if x3p else (a_ptr, -lda if a_trans else lda)) + (x_ptr, _opt(X2)) + epi + pooled + (
            y_ptr, int(y_rows), _opt(stats))
    with torch.cuda.device(X.device), prof.kernel("shared_mlp_gemm_%s %dx%d" % (tag, M, K),
                                                  4.0 * nb * P * (K * (2 if pro == 2 else 1) + M),
                                                  2.0 * M * K * nb * P, keyed=True, moved=moved):
        _lib.check(getattr(lib, fn)(*args, *shape), fn)
    return (Y, stats, third) if red is not None else ((Y, stats, bool(third)) if fork is not None else (Y, stats))


def bn_finalize(stats, count, gamma, beta, eps, momentum, running_mean, running_var):
    """-> (mean [C], invstd [C], coef [2,C]); updates running_mean/var in place when given."""
    _, C, tiles = stats.shape
    dev = stats.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    invstd = torch.empty(C, dtype=torch.float32, device=dev)
    coef = torch.empty((4, C), dtype=torch.float32, device=dev)      # (scale, shift, mean, invstd)
    with torch.cuda.device(dev), prof.kernel("bn_finalize", 4.0 * 2 * tiles * C):
        _lib.check(_lib.lib().usip_bn_finalize_f32(_ptr(stats), tiles, C, int(count), _opt(gamma), _opt(beta),
                                                   float(eps), float(momentum), _opt(running_mean),
                                                   _opt(running_var), _ptr(mean), _ptr(invstd), _ptr(coef),
                                                   _stream(stats)), "usip_bn_finalize_f32")
    # the f32x2 kernels bound |relu(bn(y))| by |gamma| sqrt(n) + |beta| with n = the samples of THEIR launch; that holds
    # when the statistics were taken over no more samples than that (bound_covers)
    declare_samples(coef, int(count))
    return mean, invstd, coef


# data_ptr of a [4,C] forward-coefficient tensor -> (the number of samples its statistics were taken over, its element
# count).  Keyed by ADDRESS, not by a Python attribute: the tensor a backward pass gets back from ctx.saved_tensors, a detach()
# or a row view is another Python object over the same memory, and an attribute would be gone.  bn_finalize
# re-declares on every call, so an address that the allocator hands out again carries its newest producer's count; a
# hand-built tensor of ANOTHER size that lands on a recycled address does not inherit the old count (the element count is
# checked: ADVICE r5), and the table sheds its OLDEST entries (a step declares a few dozen: nothing of a running step's
# forward is dropped before its backward) instead of being cleared.
import collections
_SAMPLES = collections.OrderedDict()
_SAMPLES_MAX = 8192
UNKNOWN_SAMPLE_LOOKUPS = 0          # bound_covers calls that found no recorded count (a whole step must leave this at 0)


def declare_samples(coef, count: int):
    """Record that the batch statistics in `coef` were taken over `count` samples per channel."""
    key = coef.data_ptr()
    _SAMPLES.pop(key, None)
    _SAMPLES[key] = (int(count), int(coef.numel()))           # (re-)inserted at the young end
    while len(_SAMPLES) > _SAMPLES_MAX:
        _SAMPLES.popitem(last=False)


def bound_covers(coef, samples: int) -> bool:
    """May a launch over `samples` positions per channel use the BatchNorm bound of `coef` (its [4,C] batch
    statistics)?  |y - mean| <= sqrt(n var) holds over the n samples the statistics were taken over; a launch that
    assumes n' = its own sample count under-estimates the bound when n' < n (a slice of the tensor, coefficients of
    another batch) and could overflow the fp16 planes.  Coefficients WITHOUT a recorded count do not cover anything
    (the launch takes the bound-free f32x3 path); hand-built coefficients in tests and tools either call
    declare_samples or set USIP_ASSUME_LAUNCH_SAMPLES=1 (the `assume_launch_samples` fixture of tests/conftest.py), which takes
    them as the launch's own."""
    global UNKNOWN_SAMPLE_LOOKUPS
    rec = _SAMPLES.get(coef.data_ptr())
    if rec is not None and rec[1] != int(coef.numel()) and coef._base is None:
        rec = None                  # another tensor on a recycled address (a view of the declared one keeps its base's count)
    if rec is None:
        UNKNOWN_SAMPLE_LOOKUPS += 1
        return os.environ.get("USIP_ASSUME_LAUNCH_SAMPLES") == "1"
    return rec[0] <= samples


def bn_apply(Y, coef, relu: bool):
    """Z = relu?(Y * coef[0] + coef[1]); Y [nb,C,P]."""
    nb, C, P = Y.shape
    Z = torch.empty_like(Y)
    with torch.cuda.device(Y.device), prof.kernel("bn_apply", 8.0 * nb * C * P):
        _lib.check(_lib.lib().usip_bn_apply_f32(_ptr(Y), _ptr(coef), _ptr(Z), int(bool(relu)), nb, C, P,
                                                _stream(Y)), "usip_bn_apply_f32")
    return Z


def bn_backward_reduce(dZ, Y, coef_fwd, mean, invstd, gamma, relu: bool, group: int = 0,
                       dgamma_out=None, dbeta_out=None):
    """-> (dgamma [C], dbeta [C], coef4 [4,C], gsum).  Y None: plain mode, returns (None, sum dZ, None, None).
    group > 0 additionally returns gsum [2,nb,C,P/group] (per-neighbourhood sums of dYhat and y)."""
    nb, C, P = dZ.shape
    dev = dZ.device
    # f32x2 mode: the pass also takes max |dYhat| per row and leaves a bound of |dY| in row 4 of coef4 ([5][C])
    want_bound = 1 if (_matmul_mode == "f32x2" and Y is not None) else 0
    partial = torch.empty((3 if want_bound else 2) * nb * C, dtype=torch.float32, device=dev)
    dbeta = dbeta_out if dbeta_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = coef4 = gsum = None
    if Y is not None:
        dgamma = dgamma_out if dgamma_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
        coef4 = torch.empty((5 if want_bound else 4, C), dtype=torch.float32, device=dev)
        if group:
            gsum = torch.empty((2, nb, C, P // group), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), prof.kernel("bn_backward_reduce", 4.0 * nb * C * P * (1 if Y is None else 2)):
        _lib.check(_lib.lib().usip_bn_backward_reduce_f32(_ptr(dZ), _opt(Y), _opt(coef_fwd), _opt(mean), _opt(invstd),
                                                          _opt(gamma), int(bool(relu)), _ptr(partial), _opt(dgamma),
                                                          _ptr(dbeta), _opt(coef4), _opt(gsum), int(group),
                                                          nb, C, P, want_bound, _stream(dZ)),
                   "usip_bn_backward_reduce_f32")
    return dgamma, dbeta, coef4, gsum


def bn_backward_reduce_wide(dZ, Y, coef_fwd, mean, invstd, gamma, relu: bool, group: int,
                            dgamma_out=None, dbeta_out=None, want_bound=None, want_partial: bool = False):
    """bn_backward_reduce(group=...) for group % 4 == 0, 256 < group <= 1024 -> (dgamma [C], dbeta [C], coef4, gsum
    [2,nb,C,P/group]); want_bound None: as the matmul mode asks.  want_partial: the per-row partial sums as a fifth value."""
    nb, C, P = dZ.shape
    dev = dZ.device
    if want_bound is None:
        want_bound = _matmul_mode == "f32x2"
    want_bound = int(bool(want_bound))
    if group <= 0 or P % group:
        raise RuntimeError("bn_backward_reduce_wide: P = %d is no multiple of group = %d" % (P, group))
    partial = torch.empty((3 if want_bound else 2) * nb * C, dtype=torch.float32, device=dev)
    dbeta = dbeta_out if dbeta_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = dgamma_out if dgamma_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    coef4 = torch.empty((5 if want_bound else 4, C), dtype=torch.float32, device=dev)
    gsum = torch.empty((2, nb, C, P // group), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), prof.kernel("bn_backward_reduce_wide", 8.0 * nb * C * P):
        _lib.check(_lib.lib().usip_bn_backward_reduce_wide_f32(_opt(dZ), _opt(Y), _opt(coef_fwd), _opt(mean),
                                                               _opt(invstd), _opt(gamma), int(bool(relu)), _ptr(partial),
                                                               _ptr(dgamma), _ptr(dbeta), _ptr(coef4), _ptr(gsum),
                                                               int(group), nb, C, P, want_bound, _stream(dZ)),
                   "usip_bn_backward_reduce_wide_f32")
    return (dgamma, dbeta, coef4, gsum, partial) if want_partial else (dgamma, dbeta, coef4, gsum)


# Deferred weight-gradient reductions (include/usip_hip.h: usip_wgrad_defer / usip_wgrad_flush): inside a training step the
# fixed-order sums of partial tiles are recorded by the library and issued together after backward.  The partial-tile
# workspaces must outlive the flush, so while the mode is on every workspace allocated here is kept in _DEFER_KEEP.
_DEFER_KEEP = None


def _keep(ws):
    if _DEFER_KEEP is not None:
        _DEFER_KEEP.append(ws)
    return ws


def wgrad_defer(on: bool, device=None):
    """Enter (True) or leave (False) the deferred mode; leaving drops whatever is recorded and not flushed.
    device: record only what is launched on that device's CURRENT stream (the step's); anything another thread, device or
    stream launches meanwhile runs its reduction at once (the library's job list is process-global)."""
    global _DEFER_KEEP
    if on and device is not None:
        dev = torch.device(device)
        _lib.check(_lib.lib().usip_wgrad_defer_on(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "usip_wgrad_defer_on")
    else:
        _lib.check(_lib.lib().usip_wgrad_defer(1 if on else 0), "usip_wgrad_defer")
    _DEFER_KEEP = [] if on else None


class _reduce_now:
    """`with _reduce_now(dest_is_private):` -- a weight gradient whose destination is NOT handed in by the caller (no view of
    the step's gradient bucket: a frozen sibling parameter switched the layer's sink off, functional._sink) goes back to
    autograd, whose AccumulateGrad reads it before any flush: its fixed-order sum must be launched at once."""

    def __init__(self, private: bool):
        self.on = bool(private) and _DEFER_KEEP is not None

    def __enter__(self):
        if self.on:
            self.was = int(_lib.lib().usip_wgrad_defer_hold(1))

    def __exit__(self, *exc):
        if self.on:
            _lib.lib().usip_wgrad_defer_hold(self.was)
        return False


def wgrad_flush(device) -> int:
    """Issue every recorded reduction on `device`'s current stream (two launches at most); -> how many were issued.
    The mode stays on; the workspaces are released (stream-ordered: their memory is reused only behind the flush)."""
    global _DEFER_KEEP
    dev = torch.device(device)
    with torch.cuda.device(dev), prof.kernel("wgrad_reduce_all", 0.0):
        n = int(_lib.lib().usip_wgrad_flush(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    if n < 0:
        raise RuntimeError("usip_amd: usip_wgrad_flush failed (%d)" % n)
    if _DEFER_KEEP is not None:
        _DEFER_KEEP = []
    return n


def bn_pool_backward_reduce(dpooled, arg, Y4, coef_fwd, mean, invstd, gamma, relu: bool,
                            dgamma_out=None, dbeta_out=None, yarg=None):
    """BN(+ReLU) backward sums for a layer that fed only a max over K: -> (dgamma, dbeta, coef4).
    yarg: Y4 at the arg-max as group_max_act(..., want_yarg=True) returned it (saves the gathers)."""
    nb, C, M, K = Y4.shape
    dev = Y4.device
    want_bound = 1 if _matmul_mode == "f32x2" else 0
    partial = torch.empty((3 if want_bound else 2) * nb * C, dtype=torch.float32, device=dev)
    dbeta = dbeta_out if dbeta_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dgamma = dgamma_out if dgamma_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    coef4 = torch.empty((5 if want_bound else 4, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), prof.kernel("bn_backward_reduce_pooled", 4.0 * nb * C * M * 3):
        _lib.check(_lib.lib().usip_bn_pool_backward_reduce_f32(_ptr(dpooled), _ptr(arg), _ptr(Y4), _opt(yarg),
                                                               _ptr(coef_fwd), _ptr(mean), _ptr(invstd), _opt(gamma),
                                                               int(bool(relu)), _ptr(partial), _ptr(dgamma), _ptr(dbeta),
                                                               _ptr(coef4), nb, C, M, K, want_bound, _stream(Y4)),
                   "usip_bn_pool_backward_reduce_f32")
    return dgamma, dbeta, coef4


def mlp_wgrad(G, X, pro: int = 0, G2=None, coef4=None, out=None, coloff: int = 0, xcoef=None, pool=None):
    """dW [M,N] = sum_{b,p} pro(G)[b,m,p] * X[b,n,p]; G [nb,M,P], X [nb,N,P].
    With `out` ([M, ldw] contiguous) the result is written into columns [coloff, coloff+N) of it."""
    pool_dp = pool_arg = None
    pool_group = 0
    if pool is not None:                      # pro == 3: G is not a tensor
        pool_dp, pool_arg, pool_group = pool
        nb, M, P = G2.shape
    else:
        nb, M, P = G.shape
    N = X.shape[1]
    dev = X.device
    ws_n = _lib.lib().usip_mlp_wgrad_workspace(M, N, P, nb)
    ws = _keep(torch.empty(max(int(ws_n), 1), dtype=torch.float32, device=dev))
    dW = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=dev)
    ldw = dW.shape[1]
    fn_name = {"bf16": "usip_mlp_wgrad_bf16", "f32x3": "usip_mlp_wgrad_f32x3",
               "f32x2": "usip_mlp_wgrad_f32x3"}.get(_matmul_mode, "usip_mlp_wgrad_f32")
    x3 = _x3_family() and not (M <= 64 and N <= 64) and bool(_lib.lib().usip_mlp_wgrad_f32x3_used(M, N, P, nb))
    # two fp16 planes: both operands need a bound (coef4 with its fifth row, xcoef = batch statistics)
    x2h = (x3 and _matmul_mode == "f32x2" and pro >= 2 and coef4 is not None and coef4.shape[0] >= 5 and M > 128 and N > 128
           and xcoef is not None and xcoef.shape[0] >= 4 and P % 4 == 0 and bound_covers(xcoef, nb * P))
    if x2h:
        fn_name = "usip_mlp_wgrad_x2h_f32"

    with torch.cuda.device(dev), _reduce_now(out is None), prof.kernel(
            "shared_mlp_wgrad %dx%d" % (M, N), 4.0 * nb * P * (M * (2 if pro == 2 else 1) + N), 2.0 * M * N * nb * P,
            keyed=True):
        _lib.check(getattr(_lib.lib(), fn_name)(_opt(G), _opt(G2), _opt(coef4), int(pro), _ptr(X), _opt(xcoef),
                                                _opt(pool_dp), _opt(pool_arg), int(pool_group), _ptr(ws), _ptr(dW),
                                                int(ldw), int(coloff), M, N, P, nb, _stream(X)), fn_name)
    return dW


reduce_now = _reduce_now          # for callers that hand a PRIVATE destination through `out` / `dw_out` (functional.py)


class RedSums:
    """What a fused layer backward leaves for the layer that produced its input: `sums` [2, blocks, C] partial
    BatchNorm-backward sums and `maxima` [blocks] of |dX [relu on]| -- views of one flat buffer."""

    def __init__(self, flat: torch.Tensor, C: int, blocks: Optional[int] = None):
        """blocks: rows of the partial sums when the buffer holds another number of maxima than that (the direct GEMM's
        data-gradient epilogue: one maximum per 256-row tile)."""
        if blocks is None:
            blocks = flat.numel() // (2 * C + 1)
        self.flat = flat
        self.sums = flat[:2 * blocks * C].view(2, blocks, C)
        self.maxima = flat[2 * blocks * C:]
        self.gsum = None                     # per-neighbourhood sums [2,nb,C,G], when the producer took them too
        self.wsum = None                     # (wsum, wsum3, source tensor): the producing layer's weight-gradient sums (WSUM)


def narrow_backward_supported(Cin: int, Cout: int, P: int, tensors=()) -> bool:
    """True when usip_mlp_narrow_backward_f32 takes this layer.  `tensors`: the (dZ, Y, X) the call would pass --
    the kernel needs them 16-byte aligned (an offset view handed over by autograd is not) and addresses elements
    with 32-bit offsets; anything else goes through the generic data- and weight-gradient kernels instead of
    raising in the middle of a backward."""
    if _matmul_mode == "bf16" or not _lib.lib().usip_mlp_narrow_backward_supported(int(Cin), int(Cout), int(P)):
        return False
    for t in tensors:
        if t is None:
            continue
        if t.data_ptr() % 16 != 0 or t.numel() >= 2 ** 32 or not t.is_contiguous():
            return False
    return True


def mlp_narrow_backward(dz, y, coef4, x, xcoef, w2, wcol: int = 0, dw_out=None, Cin: int = 64, want_red: bool = False):
    """Fused backward of a narrow layer (csrc/narrow_bwd.hip): -> (dx [nb,Cin,P], dW[, red]).
    dz, y [nb,Cout,P]; x [nb,Cin,P]; w2 [Cout, Ctot] contiguous, the layer's inputs are its columns [wcol, wcol+Cin);
    dw_out ([Cout, Ctot] contiguous) receives the weight gradient in the same columns.
    want_red (xcoef = the producing layer's [4,Cin] forward coefficients): also returns a RedSums: partial
    BatchNorm-backward sums [2, blocks, Cin] of the producing layer against dx and the workgroups' maxima of
    |dx [relu on]| (see bn_backward_from_partials)."""
    nb, Cout, P = dz.shape
    dev = dz.device
    for t, n in ((dz, "dz"), (y, "y"), (x, "x"), (w2, "w2"), (coef4, "coef4")):
        _need(t, n, torch.float32)
    ldw = w2.shape[1]
    dW = dw_out if dw_out is not None else torch.empty_like(w2)
    dx = torch.empty((nb, Cin, P), dtype=torch.float32, device=dev)
    ws = _keep(torch.empty(int(_lib.lib().usip_mlp_narrow_backward_workspace(Cout, P, nb)), dtype=torch.float32, device=dev))
    red = None
    if want_red:
        if xcoef is None or xcoef.shape[0] < 4:
            raise RuntimeError("mlp_narrow_backward: want_red needs the producing layer's [4, Cin] coefficients")
        blocks = int(_lib.lib().usip_mlp_narrow_backward_blocks(Cout, P, nb))
        red = torch.empty(2 * blocks * Cin + blocks, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _reduce_now(dw_out is None), prof.kernel("shared_mlp_narrow_bwd %dx%d" % (Cout, Cin),
                                             4.0 * nb * P * (2 * Cout + 2 * Cin), 4.0 * Cout * Cin * nb * P, keyed=True):
        _lib.check(_lib.lib().usip_mlp_narrow_backward_f32(
            _ptr(dz), _ptr(y), _ptr(coef4), _ptr(x), int(x.shape[1]), _opt(xcoef),
            ctypes.c_void_p(w2.data_ptr() + 4 * int(wcol)), int(ldw), _ptr(dx), Cin, _ptr(ws),
            ctypes.c_void_p(dW.data_ptr() + 4 * int(wcol)), int(dW.shape[1]), _opt(red), Cin, Cout, P, nb, _stream(dz)),
            "usip_mlp_narrow_backward_f32")
    return (dx, dW, RedSums(red, Cin)) if want_red else (dx, dW)


def layer_backward_x2_supported(Cin: int, Cout: int, P: int, tensors=(), coef4=None, xcoef=None, pooled: bool = False) -> bool:
    """True when usip_mlp_layer_backward_x2h_f32 takes this layer: f32x2 mode, a supported shape, the bounds the two
    fp16 planes need (coef4 with its fifth row, the producing layer's four-row coefficients), aligned contiguous tensors."""
    if _matmul_mode != "f32x2" or not LAYER_BWD_X2:
        return False
    if coef4 is None or coef4.shape[0] < 5 or xcoef is None or xcoef.shape[0] < 4:
        return False
    nb = next((t.shape[0] for t in tensors if t is not None and t.dim() == 3), None)
    if nb is not None and not bound_covers(xcoef, int(nb) * int(P)):
        return False
    if not _lib.lib().usip_mlp_layer_backward_x2h_supported(int(Cin), int(Cout), int(P), 1 if pooled else 0):
        return False
    for t in tensors:
        if t is None:
            continue
        if t.data_ptr() % 16 != 0 or t.numel() >= 2 ** 32 or not t.is_contiguous():
            return False
    return True


# f32x2 mode: the fused layer backward on the 16-bit matrix cores; USIP_LAYER_BWD_X2=0 for A/B runs
LAYER_BWD_X2 = _os.environ.get("USIP_LAYER_BWD_X2", "1") not in ("0", "off")


def mlp_layer_backward_x2(dz, y, coef4, x, xcoef, w2, wcol: int = 0, dw_out=None, Cin: int = 64, want_red: bool = False,
                          pool=None, want_gsum: bool = False, wsrc=None):
    """Fused backward of a <= 128-wide layer with f32x2 products (csrc/layer_bwd_x2.hip): -> (dx [nb,Cin,P], dW[, red]).
    Arguments as mlp_narrow_backward; coef4 [5,Cout] (with bounds), xcoef [4,Cin]; pool = (dpooled [nb,Cout,G],
    arg i32 [nb,Cout,G], group) with dz None for the pooled form.  red: a RedSums (partial sums [2, blocks, Cin] and the
    workgroups' maxima of |dx [relu on]|); want_gsum (pooled form with red, group % 32 == 0): red.gsum [2,nb,Cin,G] =
    the per-neighbourhood sums of dx [relu on] and of x that bn_backward_reduce(group=...) would return.
    wsrc ([nb, <= 8, P], the gradient-free INPUT of the layer that produced x; (64, 64) form with want_red): red.wsum = the
    sums that layer's weight gradient follows from (wsum_finalize) -- it then needs no pass over its own (dZ, Y)."""
    nb, Cout, P = y.shape
    dev = y.device
    for t, n in ((y, "y"), (x, "x"), (w2, "w2"), (coef4, "coef4"), (xcoef, "xcoef")):
        _need(t, n, torch.float32)
    ldw = w2.shape[1]
    dW = dw_out if dw_out is not None else torch.empty_like(w2)
    dx = torch.empty((nb, Cin, P), dtype=torch.float32, device=dev)
    lib = _lib.lib()
    blocks = int(lib.usip_mlp_layer_backward_x2h_blocks(Cin, Cout, P, nb))
    ws = _keep(torch.empty(int(lib.usip_mlp_layer_backward_x2h_workspace(Cin, Cout, P, nb)), dtype=torch.float32, device=dev))
    red = torch.empty(2 * blocks * Cin + blocks, dtype=torch.float32, device=dev) if want_red else None
    planes = weight_planes(w2, wcol, Cin, Cout, 2, P, nb)      # W as the data-gradient operand: K-major [Cout][ldw]
    pdp = parg = gsum = None
    group = 0
    if pool is not None:
        pdp, parg, group = pool
        _need(pdp, "dpooled", torch.float32)
        _need(parg, "arg", torch.int32)
        if want_gsum:
            if not want_red or group % 32:
                raise ValueError("mlp_layer_backward_x2: group sums need want_red and a group that is a multiple of 32")
            gsum = torch.empty((2, nb, Cin, P // group), dtype=torch.float32, device=dev)
    else:
        _need(dz, "dz", torch.float32)
    wsum = wsum3 = None
    if want_red and wsum_supported(wsrc, Cin, Cout, P, pool is not None):
        wsum = torch.empty((blocks, Cin, 16), dtype=torch.float32, device=dev)
        wsum3 = torch.empty((blocks, 8), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _reduce_now(dw_out is None), prof.kernel(
            "shared_mlp_layer_bwd_x2%s %dx%d" % ("ws" if wsum is not None else "", Cout, Cin),
            4.0 * nb * P * ((1 if pool is not None else 2) * Cout + 2 * Cin + (wsrc.shape[1] if wsum is not None else 0)),
            4.0 * Cout * Cin * nb * P, keyed=True):
        if wsum is not None:
            _lib.check(lib.usip_mlp_layer_backward_x2h_ws_f32(
                _ptr(dz), _ptr(y), _ptr(coef4), _ptr(x), int(x.shape[1]), _ptr(xcoef), ctypes.c_void_p(planes.data_ptr()),
                _ptr(dx), Cin, _ptr(ws), ctypes.c_void_p(dW.data_ptr() + 4 * int(wcol)), int(dW.shape[1]), _ptr(red),
                _ptr(wsrc), int(wsrc.shape[1]), _ptr(wsum), _ptr(wsum3), Cin, Cout, P, nb, _stream(y)),
                "usip_mlp_layer_backward_x2h_ws_f32")
        else:
            _lib.check(lib.usip_mlp_layer_backward_x2h_f32(
                _opt(dz), _ptr(y), _ptr(coef4), _opt(pdp), _opt(parg), int(group), _ptr(x), int(x.shape[1]), _ptr(xcoef),
                ctypes.c_void_p(planes.data_ptr()), _ptr(dx), Cin, _ptr(ws), ctypes.c_void_p(dW.data_ptr() + 4 * int(wcol)),
                int(dW.shape[1]), _opt(red), _opt(gsum), Cin, Cout, P, nb, _stream(y)), "usip_mlp_layer_backward_x2h_f32")
    if not want_red:
        return dx, dW
    r = RedSums(red, Cin)
    r.gsum = gsum
    if wsum is not None:
        r.wsum = (wsum, wsum3, wsrc)
    return dx, dW, r


WSUM = _os.environ.get("USIP_WSUM", "1") not in ("0", "off")        # A/B switch of the fused first-layer weight gradient


def wsum_supported(wsrc, Cin: int, Cout: int, P: int, pooled: bool) -> bool:
    """May mlp_layer_backward_x2 take the producing layer's weight-gradient sums against `wsrc` on the way?"""
    return (WSUM and wsrc is not None and not pooled and Cin == 64 and Cout == 64 and wsrc.dim() == 3 and wsrc.shape[1] <= 8
            and wsrc.shape[2] == P and wsrc.is_contiguous() and wsrc.data_ptr() % 16 == 0 and wsrc.dtype == torch.float32)


def wsum_finalize(wsum_pack, coef4, mean, dW):
    """dW[:, :rows] = the weight gradient of the layer whose sums `wsum_pack` (RedSums.wsum) holds, from its own coef4 /
    batch mean (csrc/layer_bwd_x2.hip::wsum_finalize_kernel); dW [C, >= rows] contiguous rows."""
    wsum, wsum3, wsrc = wsum_pack
    blocks = wsum3.shape[0]
    C = wsum.shape[1]
    with torch.cuda.device(dW.device), prof.kernel("wsum_finalize", 4.0 * blocks * (16 * C + 8)):
        _lib.check(_lib.lib().usip_mlp_wsum_finalize_f32(_ptr(wsum), _ptr(wsum3), int(blocks), int(C), _ptr(coef4), _ptr(mean),
                                                         int(wsrc.shape[1]), _ptr(dW), int(dW.stride(0)), _stream(dW)),
                   "usip_mlp_wsum_finalize_f32")
    return dW


def bn_pool_backward_partials(dpooled, arg, Y4, coef_fwd, mean, invstd, relu: bool, yarg=None):
    """Partial BatchNorm-backward sums [2, nb, C] of a gradient that is dpooled at the arg-max positions and zero
    elsewhere (the sparse half of a layer output that feeds a max-pool AND another layer).  In f32x2 mode a RedSums
    whose maxima [nb * C] are those of |dpooled [relu on]| per cloud and channel."""
    nb, C, M, K = Y4.shape
    want_max = _matmul_mode == "f32x2"
    partial = torch.empty((3 if want_max else 2) * nb * C, dtype=torch.float32, device=Y4.device)
    with torch.cuda.device(Y4.device), prof.kernel("bn_backward_reduce_pooled", 4.0 * nb * C * M * 3):
        _lib.check(_lib.lib().usip_bn_pool_backward_reduce_f32(_ptr(dpooled), _ptr(arg), _ptr(Y4), _opt(yarg),
                                                               _ptr(coef_fwd), _ptr(mean), _ptr(invstd), None,
                                                               int(bool(relu)), _ptr(partial), None, None, None, nb, C,
                                                               M, K, 1 if want_max else 0, _stream(Y4)),
                   "usip_bn_pool_backward_reduce_f32")
    if want_max:
        r = RedSums.__new__(RedSums)
        r.flat, r.sums, r.maxima = partial, partial[:2 * nb * C].view(2, nb, C), partial[2 * nb * C:]
        return r
    return partial.view(2, nb, C)


def bn_backward_from_partials(partials, count: int, coef_fwd, mean, invstd, dgamma_out=None, dbeta_out=None):
    """(dgamma, dbeta, coef4) from partial sums [2, rows, C] (one tensor / RedSums or a list of them: all are summed).
    When every part is a RedSums (at most two) coef4 gets its fifth row, the bound of |dY| the f32x2 kernels need:
    |dYhat| <= the sum of the parts' maxima."""
    parts = list(partials) if isinstance(partials, (list, tuple)) else [partials]
    maxima = [p.maxima for p in parts] if all(isinstance(p, RedSums) for p in parts) and len(parts) <= 2 else None
    sums = [p.sums if isinstance(p, RedSums) else p for p in parts]
    sums = torch.cat(sums, dim=1).contiguous() if len(sums) > 1 else sums[0]
    _, rows, C = sums.shape
    dev = sums.device
    dgamma = dgamma_out if dgamma_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = dbeta_out if dbeta_out is not None else torch.empty(C, dtype=torch.float32, device=dev)
    coef4 = torch.empty((5 if maxima else 4, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), prof.kernel("bn_backward_finalize", 8.0 * rows * C):
        if maxima:
            m1 = maxima[1] if len(maxima) > 1 else None
            _lib.check(_lib.lib().usip_bn_backward_finalize_max_f32(
                _ptr(sums), int(rows), int(C), int(count), _ptr(coef_fwd), _ptr(mean), _ptr(invstd), _ptr(dgamma),
                _ptr(dbeta), _ptr(coef4), _ptr(maxima[0]), int(maxima[0].numel()), _opt(m1),
                0 if m1 is None else int(m1.numel()), _stream(sums)), "usip_bn_backward_finalize_max_f32")
        else:
            _lib.check(_lib.lib().usip_bn_backward_finalize_f32(_ptr(sums), int(rows), int(C), int(count), _ptr(coef_fwd),
                                                                _ptr(mean), _ptr(invstd), _ptr(dgamma), _ptr(dbeta),
                                                                _ptr(coef4), _stream(sums)),
                       "usip_bn_backward_finalize_f32")
    return dgamma, dbeta, coef4


# --------------------------------------------------------------------------- grouping / pooling
def group_gather(x, idx32, sub=None, out=None, coff: int = 0):
    """out[b, coff+c, m, k] = x[b, c, idx[b,m,k]] - (c < nsub ? sub[b,c,m] : 0).  x [B,C,N], idx i32 [B,M,K],
    sub [B,nsub,M] or None.  `out` [B,Ctot,M,K] lets several gathers fill one pre-concatenated tensor."""
    _need(x, "x", torch.float32)
    _need(idx32, "idx", torch.int32)
    B, C, N = x.shape
    _, M, K = idx32.shape
    if out is None:
        out = torch.empty((B, C, M, K), dtype=torch.float32, device=x.device)
    Ctot = out.shape[1]
    nsub = 0 if sub is None else sub.shape[1]
    with torch.cuda.device(x.device), prof.kernel("group_gather", 4.0 * B * M * K * (C + 1)):
        _lib.check(_lib.lib().usip_group_gather_f32(_ptr(x), _ptr(idx32), _opt(sub), _ptr(out), B, C, N, M, K, nsub,
                                                    Ctot, int(coff), _stream(x)), "usip_group_gather_f32")
    return out


def group_gather_backward(dout, idx32, C: int, N: int, coff: int = 0):
    """dx [B,C,N] = scatter-add of dout[:, coff:coff+C] (dout [B,Ctot,M,K] contiguous)."""
    _need(dout, "dout", torch.float32)
    B, Ctot, M, K = dout.shape
    dx = torch.empty((B, C, N), dtype=torch.float32, device=dout.device)
    with torch.cuda.device(dout.device), prof.kernel("group_gather_bwd", 4.0 * B * M * K * (C + 1)):
        _lib.check(_lib.lib().usip_group_gather_backward_f32(_ptr(dout), _ptr(idx32), _ptr(dx), B, C, N, M, K, Ctot,
                                                             int(coff), _stream(dout)), "usip_group_gather_backward_f32")
    return dx


def group_max(z):
    """z [B,C,M,K] -> (pooled [B,C,M], arg i32 [B,C,M])."""
    _need(z, "z", torch.float32)
    B, C, M, K = z.shape
    pooled = torch.empty((B, C, M), dtype=torch.float32, device=z.device)
    arg = torch.empty((B, C, M), dtype=torch.int32, device=z.device)
    with torch.cuda.device(z.device), prof.kernel("group_max", 4.0 * B * C * M * (K + 2)):
        _lib.check(_lib.lib().usip_group_max_f32(_ptr(z), _ptr(pooled), _ptr(arg), B * C * M, K, _stream(z)),
                   "usip_group_max_f32")
    return pooled, arg


def group_max_act(y4, coef, relu: bool, want_yarg: bool = False):
    """max_k relu?(y*coef[0]+coef[1]) straight from a layer's pre-BN output y4 [B,C,M,K] -> (pooled, arg[, yarg]);
    yarg = y4 at the arg-max."""
    _need(y4, "y", torch.float32)
    B, C, M, K = y4.shape
    pooled = torch.empty((B, C, M), dtype=torch.float32, device=y4.device)
    arg = torch.empty((B, C, M), dtype=torch.int32, device=y4.device)
    yarg = torch.empty((B, C, M), dtype=torch.float32, device=y4.device) if want_yarg else None
    with torch.cuda.device(y4.device), prof.kernel("group_max", 4.0 * B * C * M * (K + 2)):
        _lib.check(_lib.lib().usip_group_max_act_f32(_ptr(y4), _ptr(coef), int(bool(relu)), _ptr(pooled), _ptr(arg),
                                                     _opt(yarg), B, C, M, K, _stream(y4)), "usip_group_max_act_f32")
    return (pooled, arg, yarg) if want_yarg else (pooled, arg)


# USIP_WIDE_GROUPS=0: neighbourhoods wider than 256 samples go back to the forms they had before csrc/group_wide.hip (the
# activated tensor materialised and pooled by group_max_kernel<64>, the literal cat(h, expand(pooled)) in front of the
# pooled-concat layer), for A/B runs.  functional.py reads the attribute at every call, so one process can alternate.
WIDE_GROUPS = os.environ.get("USIP_WIDE_GROUPS", "1") not in ("0", "off")


def wide_group_supported(K: int) -> bool:
    """K is a neighbourhood size csrc/group_wide.hip takes AND the GEMM / layer-backward forms with a row bias or a
    pooled group take (K % 32)."""
    return bool(WIDE_GROUPS) and 256 < K <= 1024 and K % 32 == 0


def group_max_wide(y4, coef=None, relu: bool = False, want_yarg: bool = False):
    """group_max (coef None: y4 is already activated) / group_max_act for K % 4 == 0, 256 < K <= 1024
    -> (pooled, arg[, yarg])."""
    _need(y4, "y", torch.float32)
    B, C, M, K = y4.shape
    pooled = torch.empty((B, C, M), dtype=torch.float32, device=y4.device)
    arg = torch.empty((B, C, M), dtype=torch.int32, device=y4.device)
    yarg = torch.empty((B, C, M), dtype=torch.float32, device=y4.device) if want_yarg else None
    with torch.cuda.device(y4.device), prof.kernel("group_max_wide", 4.0 * B * C * M * (K + 2)):
        _lib.check(_lib.lib().usip_group_max_wide_f32(_ptr(y4), _opt(coef), int(bool(relu)), _ptr(pooled), _ptr(arg),
                                                      _opt(yarg), B, C, M, K, _stream(y4)), "usip_group_max_wide_f32")
    return (pooled, arg, yarg) if want_yarg else (pooled, arg)


def group_max_backward(dpooled, arg, K: int):
    _need(dpooled, "dpooled", torch.float32)
    B, C, M = dpooled.shape
    dz = torch.empty((B, C, M, int(K)), dtype=torch.float32, device=dpooled.device)
    with torch.cuda.device(dpooled.device), prof.kernel("group_max_bwd", 4.0 * B * C * M * (K + 2)):
        _lib.check(_lib.lib().usip_group_max_backward_f32(_ptr(dpooled), _ptr(arg), _ptr(dz), B * C * M, int(K),
                                                          _stream(dpooled)), "usip_group_max_backward_f32")
    return dz


def group_max_backward_add_(dz, dpooled, arg):
    """In place: dz[b,c,m,arg[b,c,m]] += dpooled[b,c,m]; returns dz."""
    _need(dz, "dz", torch.float32)
    _need(dpooled, "dpooled", torch.float32)
    _need(arg, "arg", torch.int32)
    B, C, M, K = dz.shape
    if dpooled.shape != (B, C, M) or arg.shape != (B, C, M):
        raise RuntimeError("group_max_backward_add_: shapes do not match")
    with torch.cuda.device(dz.device), prof.kernel("group_max_bwd_add", 4.0 * B * C * M * 4):
        _lib.check(_lib.lib().usip_group_max_backward_add_f32(_ptr(dpooled), _ptr(arg), _ptr(dz), B * C * M, int(K),
                                                              _stream(dz)), "usip_group_max_backward_add_f32")
    return dz


def multi_transpose(src_flat, dst_flat, table, total_tiles: int):
    """K-major copies of all weight matrices described by `table` (int32 [n,5]: source offset, rows, cols,
    destination offset, first tile) from src_flat into dst_flat, one launch."""
    _need(src_flat, "src", torch.float32)
    _need(dst_flat, "dst", torch.float32)
    _need(table, "table", torch.int32)
    with torch.cuda.device(src_flat.device), prof.kernel("weight_transposes", 8.0 * dst_flat.numel()):
        _lib.check(_lib.lib().usip_multi_transpose_f32(_ptr(src_flat), _ptr(dst_flat), _ptr(table), int(table.shape[0]),
                                                       int(total_tiles), _stream(src_flat)), "usip_multi_transpose_f32")
    return dst_flat


def nearest_nd(a: torch.Tensor, b: torch.Tensor):
    """f-1: (min_j |a_i - b_j| [B,Ma], first arg-min i32 [B,Ma]) for C-dimensional a [B,C,Ma], b [B,C,Nb<=1024]."""
    _need(a, "a", torch.float32)
    _need(b, "b", torch.float32)
    B, C, Ma = a.shape
    Nb = b.shape[2]
    d = torch.empty((B, Ma), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, Ma), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device), prof.kernel("nearest_nd", 4.0 * B * C * (Ma + Nb), 3.0 * B * C * Ma * Nb):
        _lib.check(_lib.lib().usip_nearest_nd_f32(_ptr(a), _ptr(b), _ptr(d), _ptr(arg), B, C, Ma, Nb, _stream(a)),
                   "usip_nearest_nd_f32")
    return d, arg


def nearest_backward(a, b, d, arg32, gd, need_gb: bool):
    """-> (ga [B,C,Ma], gb [B,C,Nb] or None)."""
    B, C, Ma = a.shape
    Nb = b.shape[2]
    ga = torch.empty_like(a)
    gb = torch.empty_like(b) if need_gb else None
    with torch.cuda.device(a.device), prof.kernel("nearest_bwd", 4.0 * B * Ma * 12):
        _lib.check(_lib.lib().usip_nearest_backward_f32(_ptr(a), _ptr(b), _ptr(d), _ptr(arg32), _ptr(gd), _ptr(ga),
                                                        _opt(gb), B, C, Ma, Nb, _stream(a)),
                   "usip_nearest_backward_f32")
    return ga, gb


def knn(query: torch.Tensor, database: torch.Tensor, K: int) -> torch.Tensor:
    """a-7: i32 [B,M,K] nearest-first neighbour indices; query [B,3,M], database [B,3,N], N <= 1024."""
    _need_pts(query, "query")
    _need_pts(database, "database")
    B, _, M = query.shape
    N = database.shape[2]
    out = torch.empty((B, M, int(K)), dtype=torch.int32, device=query.device)
    with torch.cuda.device(query.device), prof.kernel("knn", 4.0 * B * (3 * (M + N) + M * K), 8.0 * B * M * N):
        _lib.check(_lib.lib().usip_knn_f32(_ptr(query), _ptr(database), _ptr(out), B, M, N, int(K), _stream(query)),
                   "usip_knn_f32")
    return out


def knn_layer_supported(N: int, M: int, K: int) -> bool:
    return bool(_lib.lib().usip_knn_layer_supported(int(N), int(M), int(K)))


def knn_layer_forward(U, weight2, database, query, idx32, want_stats: bool = True):
    """Y[b,co,m,k] = W[co,:3] . (database[b,:,n] - query[b,:,m]) + U[b,co,n], n = idx[b,m,k] (csrc/knn_layer.hip).
    U [B,Cout,N] (= W[:,3:] . feat + bias), weight2 [Cout,3+C] -> (Y [B,Cout,M*K], stats [2*Cout*B] or None)."""
    _need(U, "U", torch.float32)
    _need(weight2, "weight", torch.float32)
    _need_pts(query, "query")
    _need_pts(database, "database")
    _need(idx32, "idx", torch.int32)
    B, Cout, N = U.shape
    _, M, K = idx32.shape
    Y = torch.empty((B, Cout, M * K), dtype=torch.float32, device=U.device)
    stats = torch.empty(2 * Cout * B, dtype=torch.float32, device=U.device) if want_stats else None
    with torch.cuda.device(U.device), prof.kernel("knn_layer_fwd", 4.0 * B * (M * K * (Cout + 1) + Cout * N)):
        _lib.check(_lib.lib().usip_knn_layer_forward_f32(_ptr(U), _ptr(weight2), int(weight2.stride(0)), _ptr(database),
                                                         _ptr(query), _ptr(idx32), _ptr(Y), _opt(stats), B, Cout, N, M, K,
                                                         _stream(U)), "usip_knn_layer_forward_f32")
    return Y, stats


def knn_layer_backward(dZ, Y, coef4, relu: bool, dcoord, start, perm, M: int, K: int):
    """-> (dU [B,Cout,N], dWc [Cout,3]): segment sums of dY = BN'(dZ, Y) in CSR list order, and the gradient of the three
    coordinate columns of the weight (per-cloud partials added in cloud order).  dcoord [B,3,M*K] = the decentered
    neighbour coordinates (group_gather(database, idx, sub=query))."""
    _need(dZ, "dZ", torch.float32)
    _need(Y, "Y", torch.float32)
    _need(dcoord, "dcoord", torch.float32)
    B, Cout, P = Y.shape
    N = start.shape[1] - 1
    dU = torch.empty((B, Cout, N), dtype=torch.float32, device=Y.device)
    part = torch.empty((B, Cout, 3), dtype=torch.float32, device=Y.device)
    with torch.cuda.device(Y.device), prof.kernel("knn_layer_bwd", 4.0 * B * (P * (2 * Cout + 3) + Cout * N)):
        _lib.check(_lib.lib().usip_knn_layer_backward_f32(_ptr(dZ), _ptr(Y), _ptr(coef4), int(bool(relu)), _ptr(dcoord),
                                                          _ptr(start), _ptr(perm), _ptr(dU), _ptr(part), B, Cout, N,
                                                          int(M), int(K), _stream(Y)), "usip_knn_layer_backward_f32")
    return dU, part.sum(dim=0)


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr: float, beta1: float, beta2: float, eps: float, hyper=None):
    """One Adam step on flat fp32 buffers, in place (usip_adam_step_f32); `step` is a device float[1], incremented.
    hyper: device float[4] = (lr, beta1, beta2, eps) read by the kernel instead of the scalar arguments (a captured launch
    then follows a changed learning rate)."""
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (step, "step")):
        _need(t, n, torch.float32)
    n = param.numel()
    if hyper is not None:
        _need(hyper, "hyper", torch.float32)
        with torch.cuda.device(param.device), prof.kernel("adam", 4.0 * 7 * n):
            _lib.check(_lib.lib().usip_adam_step_hyper_f32(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                                           _ptr(step), _ptr(hyper), n, _stream(param)),
                       "usip_adam_step_hyper_f32")
        return
    with torch.cuda.device(param.device), prof.kernel("adam", 4.0 * 7 * n):
        _lib.check(_lib.lib().usip_adam_step_f32(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(step),
                                                 float(lr), float(beta1), float(beta2), float(eps), n, _stream(param)),
                   "usip_adam_step_f32")


def knn_points(node: torch.Tensor, x: torch.Tensor, K: int) -> torch.Tensor:
    """RPN_Detector_KNN's neighbourhoods (models/networks.py:576-581): i32 [B,M,K], the K cloud points nearest to every
    node, nearest first, ties towards the lower index.  node [B,3,M], x [B,3,N], N <= 16384, K <= min(N, 256)."""
    _need_pts(node, "node")
    _need_pts(x, "x")
    B, _, M = node.shape
    N = x.shape[2]
    out = torch.empty((B, M, K), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device), prof.kernel("knn_points", 4.0 * B * (3 * N + 3 * M + M * K)):
        _lib.check(_lib.lib().usip_knn_points_f32(_ptr(node), _ptr(x), _ptr(out), B, M, N, int(K), _stream(x)),
                   "usip_knn_points_f32")
    return out


def fps(pts: torch.Tensor, first_idx: torch.Tensor, k: int) -> torch.Tensor:
    """f-3: farthest-point sampling. pts f32 [B,3,n], first_idx i32 [B] -> i32 [B,k] indices."""
    _need_pts(pts, "pts")
    _need(first_idx, "first_idx", torch.int32)
    B, _, n = pts.shape
    out = torch.empty((B, int(k)), dtype=torch.int32, device=pts.device)
    with torch.cuda.device(pts.device), prof.kernel("fps", 12.0 * B * n, 8.0 * B * n * k):
        _lib.check(_lib.lib().usip_fps_f32(_ptr(pts), _ptr(first_idx), _ptr(out), B, n, int(k), _stream(pts)),
                   "usip_fps_f32")
    return out


def nms(keypoints: torch.Tensor, sigmas: torch.Tensor, radius: float):
    """f-4: greedy NMS by sigma. keypoints f32 [B,3,M], sigmas f32 [B,M] -> (order i32 [B,M], count i32 [B])."""
    _need_pts(keypoints, "keypoints")
    _need(sigmas, "sigmas", torch.float32)
    B, _, M = keypoints.shape
    order = torch.zeros((B, M), dtype=torch.int32, device=keypoints.device)
    count = torch.empty((B,), dtype=torch.int32, device=keypoints.device)
    with torch.cuda.device(keypoints.device), prof.kernel("nms", 16.0 * B * M):
        _lib.check(_lib.lib().usip_nms_f32(_ptr(keypoints), _ptr(sigmas), float(radius), _ptr(order), _ptr(count),
                                           B, M, _stream(keypoints)), "usip_nms_f32")
    return order, count


def ball_query_cpu(dist: torch.Tensor, radius: float, K: int) -> torch.Tensor:
    """Host twin of ball_query (BASELINE configs[0], the CPU plumbing case): dist f32 [B,M,N] on the HOST -> i32 [B,M,K]."""
    if dist.is_cuda or not dist.is_contiguous() or dist.dtype != torch.float32 or dist.dim() != 3:
        raise RuntimeError("node_to_point_dist must be a contiguous CPU float32 tensor [B,M,N]")
    B, M, N = dist.shape
    out = torch.empty((B, M, int(K)), dtype=torch.int32)
    _lib.check(_lib.lib().usip_ball_query_f32_cpu(_ptr(dist), _ptr(out), float(radius), int(K), B, M, N),
               "usip_ball_query_f32_cpu")
    return out


def pairwise_dist_cpu(a: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Host twin of pairwise_dist: a [B,3,M], x [B,3,N] on the HOST -> [B,M,N]."""
    for t, name in ((a, "a"), (x, "x")):
        if t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or t.dim() != 3 or t.shape[1] != 3:
            raise RuntimeError("%s must be a contiguous CPU float32 tensor [B,3,*]" % name)
    B, _, M = a.shape
    N = x.shape[2]
    out = torch.empty((B, M, N), dtype=torch.float32)
    _lib.check(_lib.lib().usip_pairwise_dist_f32_cpu(_ptr(a), _ptr(x), _ptr(out), B, M, N), "usip_pairwise_dist_f32_cpu")
    return out


def index_max_cpu(data: torch.Tensor, index: torch.Tensor, K: int, num_threads: int = 1) -> torch.Tensor:
    """index_max.forward_cpu / forward_multi_thread_cpu (index_max.cpp:33-112): HOST tensors."""
    for t, name, dt in ((data, "data", torch.float32), (index, "index", torch.int32)):
        if t.is_cuda or not t.is_contiguous() or t.dtype != dt:
            raise RuntimeError("%s must be a contiguous CPU %s tensor" % (name, dt))
    B, C, N = data.shape
    out = torch.empty((B, C, int(K)), dtype=torch.int32)
    _lib.check(_lib.lib().usip_index_max_f32_cpu(_ptr(data), _ptr(index), _ptr(out), B, C, N, int(K),
                                                 int(num_threads)), "usip_index_max_f32_cpu")
    return out


# --------------------------------------------------------------- f-5, f-8, f-26, f-27: batches of clouds from a bank
# Four builders (detector pairs, descriptor pairs, indoor pairs, evaluation fragments) over csrc/cloud_stage.h.  Each
# states what is its own in one CloudBatchSpec; cloud_batch checks and launches any of them, the struct fillers serve it
# and the host twins (usip_amd.pairs.host_twin) alike.  The structs that go by address are the header's own
# (include/usip_hip.h and the headers it includes), read by _lib: their fields are documented there.
class CloudBatchSpec(NamedTuple):
    ids: str                 # what an id of a call names: "scan", "sample", "fragment"
    tag: str                 # usip_<tag>_build_f32 / _apply_f32 / _build_f32_cpu / _workspace_bytes / _workspace_offset
    out_c: type              # the header's out struct,
    bank_c: Optional[type]   # bank struct (None: the bank goes as plain arguments)
    draws_c: type            # and draws struct
    bank: dict               # the bank's tensors -> dtype
    bank_meta: Optional[Callable]   # (bank struct, bank dict): the bank's own refusals and counts
    lead: Callable           # (ptr, bank dict, bank struct, ids, n, ids_host, on_device) -> the C call's leading arguments
    keys: tuple              # the outputs, in the out struct's order
    out_fields: tuple        # (output key, the out struct's field, index in it or None), in the struct's order
    table: Callable          # (N, M, Cs, n) -> key -> (shape, dtype) of the outputs of a call of n ids (cached: read only)
    draws: dict              # draw -> dtype
    draw_fields: tuple       # (draw, whether its field is in the draws struct's nested f-5 `cloud`)
    draw_shapes: Callable    # (cloud recipe, n) -> draw -> the header's layout (None: any extent)
    required: tuple          # the draws that may not be absent
    index_lead: Callable     # n -> the leading shape of rows [..., N] and node_slots [..., M]
    clouds: float            # clouds per id (the traffic estimate)


def _data_ptr(t):
    return t.data_ptr()


def _out_fields(keys, sides=(), renamed=()) -> tuple:
    """<sides[i]>_pc / _sn / _node are the out struct's pc[i] / sn[i] / node[i]; any other key is the field of its name,
    or the one `renamed` gives it."""
    cloud = {s + "_" + f: (f, i) for i, s in enumerate(sides) for f in ("pc", "sn", "node")}
    return tuple((k,) + cloud.get(k, (dict(renamed).get(k, k), None)) for k in keys)


def out_struct(spec: CloudBatchSpec, ptr, out: dict, rows, node_slots):
    """ptr: tensor or array -> address (device tensors in cloud_batch, numpy arrays in the host twins)."""
    o = spec.out_c()
    for k, field, i in spec.out_fields:
        if i is None:
            setattr(o, field, ptr(out[k]))
        else:
            getattr(o, field)[i] = ptr(out[k])
    o.rows = None if rows is None else ptr(rows)
    o.node_slots = None if node_slots is None else ptr(node_slots)
    return o


def bank_struct(spec: CloudBatchSpec, ptr, bank: dict):
    """The bank struct of bank's tensors (or arrays), its counts and min_rows, after the bank's own refusals."""
    if spec.bank_c is None:
        return None
    b = spec.bank_c()
    for k in spec.bank:
        setattr(b, k, None if bank[k] is None else ptr(bank[k]))
    b.min_rows = int(bank["min_rows"])
    spec.bank_meta(b, bank)
    return b


def _draw_fields(own=(), cloud=()) -> tuple:
    return tuple((k, False) for k in own) + tuple((k, True) for k in cloud)


def draws_struct(spec: CloudBatchSpec, ptr, draws: dict):
    d = spec.draws_c()
    for k, nested in spec.draw_fields:
        if draws.get(k) is not None:
            setattr(d.cloud if nested else d, k, ptr(draws[k]))
    if "tries" in spec.draws:                           # f-8 counts them: tries is i32 [P][T]
        d.T = int(draws["tries"].shape[1])
    return d


def cloud_recipe(recipe):
    """f-5's recipe: the struct itself, or the `cloud` a descriptor recipe nests."""
    return recipe if type(recipe) is PairsRecipeC else recipe.cloud


def check_draws(spec: CloudBatchSpec, c, n: int, draws: dict, error):
    """Every present draw in the header's layout (the kernels and the host twin index it by that layout: a shorter array
    would be read past its end); absent only where the builder allows it."""
    want = spec.draw_shapes(c, n)
    for k in spec.draws:
        t = draws.get(k)
        if t is None:
            if k in spec.required:
                raise error("%s: draw %s is missing" % (spec.tag, k))
        elif len(t.shape) != len(want[k]) or any(w is not None and s != w for s, w in zip(t.shape, want[k])):
            raise error("%s: draw %s must be %s %s, got %s" % (spec.tag, k, spec.draws[k], want[k], tuple(t.shape)))


@functools.lru_cache(maxsize=None)
def cloud_batch_entry(tag: str, what: str):
    """(the library's usip_<tag>_<what>, its name)."""
    symbol = "usip_%s_%s" % (tag, what)
    return getattr(_lib.lib(), symbol), symbol


def cloud_batch_workspace(spec: CloudBatchSpec, recipe, n: int, part=None) -> int:
    """usip_<tag>_workspace_bytes, or with `part` usip_<tag>_workspace_offset."""
    fn, symbol = cloud_batch_entry(spec.tag, "workspace_bytes" if part is None else "workspace_offset")
    got = fn(ctypes.addressof(recipe), int(n)) if part is None else fn(ctypes.addressof(recipe), int(n), int(part))
    if got < 0:
        raise RuntimeError("usip_amd: %s: invalid recipe%s (USIP_EINVAL)" % (symbol, "" if part is None else " or part"))
    return got


def counter_args(counter) -> tuple:
    """(seed, step[, pair_base]) as the entry points take them: the first two are uint64_t."""
    return (int(counter[0]) & 0xFFFFFFFFFFFFFFFF, int(counter[1]) & 0xFFFFFFFFFFFFFFFF) + tuple(map(int, counter[2:]))


def cloud_batch_table(spec: CloudBatchSpec, recipe, n: int) -> dict:
    """key -> (shape, dtype) of the outputs of a call of n ids; recipe: the struct, or anything with its N, M and Cs."""
    c = getattr(recipe, "cloud", recipe)
    return spec.table(c.N, c.M, c.Cs, n)


def cloud_batch(spec: CloudBatchSpec, recipe, bank: dict, ids: torch.Tensor, out: dict, workspace: torch.Tensor, rows=None,
                node_slots=None, counter=None, draws=None, ids_host=None):
    """One call of a builder into `out` (spec.keys -> tensors): usip_<tag>_build_f32 with Philox draws under counter =
    (seed, step[, pair_base]), or with `draws` (spec.draws -> device tensors in the header's layouts)
    usip_<tag>_apply_f32.  Every tensor the launch touches is held to the bank's device, its dtype and its shape (a
    pointer to another device's memory, or past an array's end, would be dereferenced by the kernels); nothing is
    enqueued before the last refusal."""
    tag, c, dev = spec.tag, cloud_recipe(recipe), bank["rows"].device
    for k, dt in spec.bank.items():
        _need(bank[k], "bank " + k, dt)
        if bank[k].device != dev:
            raise RuntimeError("%s: bank %s on %s, the rows on %s" % (tag, k, bank[k].device, dev))
    b = bank_struct(spec, _data_ptr, bank)
    _need(ids, "ids", torch.int32)
    n = ids.numel()
    if ids.device != dev:
        raise RuntimeError("%s: ids on %s, the bank on %s" % (tag, ids.device, dev))
    if ids_host is not None and (ids_host.dtype != "int32" or ids_host.size != n or not ids_host.flags.c_contiguous):
        raise RuntimeError("%s: ids_host must be a C-contiguous int32 numpy array of the ids" % tag)
    for k, (shape, dt) in spec.table(c.N, c.M, c.Cs, n).items():
        t = out[k]
        _need(t, k, dt)
        if t.shape != shape or t.device != dev:
            raise RuntimeError("%s: %s must be %s %s on %s" % (tag, k, dt, shape, dev))
    if workspace.device != dev or workspace.numel() * workspace.element_size() < cloud_batch_workspace(spec, recipe, n):
        raise RuntimeError("%s: the workspace must hold usip_%s_workspace_bytes() bytes on %s" % (tag, tag, dev))
    if rows is not None or node_slots is not None:
        for name, t, last in (("rows", rows, c.N), ("node_slots", node_slots, c.M)):
            if t is not None:
                _need(t, name, torch.int32)
                if tuple(t.shape) != spec.index_lead(n) + (last,) or t.device != dev:
                    raise RuntimeError("%s: %s must be i32 %s on %s" % (tag, name, spec.index_lead(n) + (last,), dev))
    kind, args = "build", [ctypes.addressof(recipe)]
    if draws is not None:
        for k, dt in spec.draws.items():
            if draws.get(k) is not None:
                _need(draws[k], "draw " + k, dt)
                if draws[k].device != dev:
                    raise RuntimeError("%s: draw %s on %s, the bank on %s" % (tag, k, draws[k].device, dev))
        check_draws(spec, c, n, draws, RuntimeError)
        d = draws_struct(spec, _data_ptr, draws)
        kind, args = "apply", args + [ctypes.addressof(d)]
    o = out_struct(spec, _data_ptr, out, rows, node_slots)
    args += spec.lead(_data_ptr, bank, b, ids.data_ptr(), n, ids_host.ctypes.data if ids_host is not None else None, True)
    args += counter_args(counter) if draws is None else ()
    args += (ctypes.addressof(o), workspace.data_ptr(), _stream(bank["rows"]))
    fn, symbol = cloud_batch_entry(tag, kind + "_f32")
    with torch.cuda.device(dev), prof.kernel(symbol[5:-4], spec.clouds * n * c.N * (32 + 4 * (3 + c.Cs))):   # "<tag>_<kind>"
        _lib.check(fn(*args), symbol)
    return out


def _cloud_table(N: int, M: int, Cs: int, n: int, a: str, b: str = None) -> dict:
    """<a>pc, sn, node (and <b>pc, sn, node) of n clouds each, float32."""
    pc, sn, node = ((n, 3, N), torch.float32), ((n, Cs, N), torch.float32), ((n, 3, M), torch.float32)
    t = {a + "pc": pc, a + "sn": sn, a + "node": node}
    if b is not None:
        t.update({b + "pc": pc, b + "sn": sn, b + "node": node})
    return t


def _shapes(spec: CloudBatchSpec, recipe, n: int) -> dict:
    return {k: shape for k, (shape, _) in cloud_batch_table(spec, recipe, n).items()}


def _table(fn):
    """A builder's table is asked for at every call, for a handful of shapes: kept per shape, handed out read-only."""
    return functools.lru_cache(maxsize=64)(lambda N, M, Cs, n: types.MappingProxyType(fn(N, M, Cs, n)))


def _f5_draw_shapes(c, n: int) -> dict:
    """include/usip_hip.h, usip_pairs_draws: per pair p and cloud at [p][c]; params f64 [P][USIP_PAIRS_NPARAM]."""
    return dict(rows=(n, 2, c.N), cand=(n, 2, c.n_sub), first=(n, 2), jit_pc=(n, 2, c.N, 3), jit_sn=(n, 2, c.N, c.Cs),
                jit_node=(n, 2, c.M, 3), params=(n, 24))


def _struct_lead(ptr, bank, b, ids, n, ids_host, on_device) -> tuple:
    return (ctypes.addressof(b), ids, n)


_F5_DRAWS = dict(rows=torch.int32, cand=torch.int32, first=torch.int32, jit_pc=torch.float64, jit_sn=torch.float64,
                 jit_node=torch.float64, params=torch.float64)
_ROWS = dict(rows=torch.float32, offsets=torch.int64)


# ---- f-5 training pairs (include/usip_hip.h): the bank goes as plain arguments, the library refuses the draws it misses
PairsRecipeC = _lib.STRUCTS["usip_pairs_recipe"]
PairsDrawsC = _lib.STRUCTS["usip_pairs_draws"]
PairsOutC = _lib.STRUCTS["usip_pairs_out"]

PAIRS_KEYS = ("src_pc", "src_sn", "src_node", "dst_pc", "dst_sn", "dst_node", "R", "scale", "shift")
PAIRS_DRAWS = _F5_DRAWS


@_table
def _pairs_table(N: int, M: int, Cs: int, P: int) -> dict:
    f = torch.float32
    return dict(_cloud_table(N, M, Cs, P, "src_", "dst_"), R=((P, 3, 3), f), scale=((P,), f), shift=((P, 3, 1), f))


def pairs_shapes(recipe, P: int) -> dict:
    """key -> shape of one batch of P pairs (all float32): what DetectorStep.step consumes."""
    return _shapes(PAIRS, recipe, P)


def _pairs_lead(ptr, bank, b, ids, n, ids_host, on_device) -> tuple:
    """bank, offsets, num_scans, scan_ids, P, and for the device entries min_rows (the host twin reads the offsets)."""
    return (ptr(bank["rows"]), ptr(bank["offsets"]), bank["offsets"].shape[0] - 1, ids, n) + \
        ((int(bank["min_rows"]),) if on_device else ())


PAIRS = CloudBatchSpec(
    ids="scan", tag="pairs", out_c=PairsOutC, bank_c=None, draws_c=PairsDrawsC, bank=_ROWS, bank_meta=None, lead=_pairs_lead,
    keys=PAIRS_KEYS, out_fields=_out_fields(PAIRS_KEYS, ("src", "dst")), table=_pairs_table, draws=PAIRS_DRAWS,
    draw_fields=_draw_fields(own=PAIRS_DRAWS),
    draw_shapes=_f5_draw_shapes, required=(), index_lead=lambda P: (2, P), clouds=2.0)


def pairs_build(recipe: PairsRecipeC, bank: torch.Tensor, offsets: torch.Tensor, scan_ids: torch.Tensor, min_rows: int,
                seed: int, step: int, pair_base: int, out: dict, workspace: torch.Tensor, rows=None, node_slots=None):
    """f-5: P training pairs with Philox draws (usip_pairs_build_f32) into `out` (PAIRS_KEYS -> f32 tensors)."""
    return cloud_batch(PAIRS, recipe, dict(rows=bank, offsets=offsets, min_rows=min_rows), scan_ids, out, workspace, rows,
                       node_slots, counter=(seed, step, pair_base))


def pairs_apply(recipe: PairsRecipeC, draws: dict, bank: torch.Tensor, offsets: torch.Tensor, scan_ids: torch.Tensor,
                min_rows: int, out: dict, workspace: torch.Tensor, rows=None, node_slots=None):
    """f-5 with explicit draws (usip_pairs_apply_f32): draws = rows, cand, first (i32), jit_pc, jit_sn, jit_node,
    params (f64) device tensors in the layouts of include/usip_hip.h."""
    return cloud_batch(PAIRS, recipe, dict(rows=bank, offsets=offsets, min_rows=min_rows), scan_ids, out, workspace, rows,
                       node_slots, draws=draws)


def pairs_workspace_offset(recipe: PairsRecipeC, P: int, part: int) -> int:
    """Byte offset of workspace part 0 table, 1 candidates, 2 first indices, 3 FPS picks, 4 total (include/usip_hip.h)."""
    return cloud_batch_workspace(PAIRS, recipe, P, part)


def pairs_workspace_bytes(recipe: PairsRecipeC, P: int) -> int:
    return cloud_batch_workspace(PAIRS, recipe, P)


# ---- f-8 descriptor batches from posed scans (recipe.cloud is a PairsRecipeC, draws.cloud a PairsDrawsC: the reader
# nests the classes); the library counts tries, so they may not be absent.  params is f-8's own [P][24] table; the nested
# cloud.params, which f-8 does not read, takes the same array so that no pointer of the struct stays NULL
DescPairsRecipeC = _lib.STRUCTS["usip_desc_pairs_recipe"]
DescPairsBankC = _lib.STRUCTS["usip_desc_pairs_bank"]
DescPairsDrawsC = _lib.STRUCTS["usip_desc_pairs_draws"]
DescPairsOutC = _lib.STRUCTS["usip_desc_pairs_out"]

DESC_PAIRS_KEYS = ("anc_pc", "anc_sn", "anc_node", "pos_pc", "pos_sn", "pos_node", "anc_pose", "pos_pose", "anc_seq",
                   "pos_id", "neg_idx", "neg_fail")
DESC_PAIRS_DRAWS = dict(_F5_DRAWS, tries=torch.int32, neg_pick=torch.int32)


@_table
def _desc_pairs_table(N: int, M: int, Cs: int, P: int) -> dict:
    f, i32 = torch.float32, torch.int32
    return dict(_cloud_table(N, M, Cs, P, "anc_", "pos_"), anc_pose=((P, 4, 4), f), pos_pose=((P, 4, 4), f),
                anc_seq=((P,), i32), pos_id=((P,), i32), neg_idx=((P,), torch.int64), neg_fail=((1,), i32))


def desc_pairs_shapes(recipe: DescPairsRecipeC, P: int) -> dict:
    """key -> (shape, dtype) of one batch of P pairs."""
    return dict(cloud_batch_table(DESC_PAIRS, recipe, P))


def _desc_pairs_bank(b: DescPairsBankC, bank: dict):
    """bank: rows, offsets, poses, seq_of, seq_start (tensors), seq_start_host (int32 numpy), min_rows."""
    S, Q, host = bank["offsets"].shape[0] - 1, bank["seq_start"].shape[0] - 1, bank["seq_start_host"]
    if tuple(bank["poses"].shape) != (S, 4, 4) or tuple(bank["seq_of"].shape) != (S,) or host.dtype != "int32" or \
            host.size != Q + 1 or not host.flags.c_contiguous:
        raise RuntimeError("desc_pairs: poses f64 (S, 4, 4), seq_of i32 (S,), seq_start i32 (num_seq + 1,) on the "
                           "device and as a C-contiguous int32 numpy array")
    b.seq_start_host, b.num_scans, b.num_seq = host.ctypes.data, S, Q


DESC_PAIRS = CloudBatchSpec(
    ids="scan", tag="desc_pairs", out_c=DescPairsOutC, bank_c=DescPairsBankC, draws_c=DescPairsDrawsC,
    bank=dict(_ROWS, poses=torch.float64, seq_of=torch.int32, seq_start=torch.int32), bank_meta=_desc_pairs_bank,
    lead=_struct_lead, keys=DESC_PAIRS_KEYS, out_fields=_out_fields(DESC_PAIRS_KEYS, ("anc", "pos")),
    table=_desc_pairs_table, draws=DESC_PAIRS_DRAWS, draw_fields=_draw_fields(own=("params", "tries", "neg_pick"), cloud=_F5_DRAWS),
    draw_shapes=lambda c, P: dict(_f5_draw_shapes(c, P), tries=(P, None), neg_pick=(P,)),
    required=("tries",), index_lead=lambda P: (2, P), clouds=2.0)


def desc_pairs_out_struct(ptr, out: dict, rows, node_slots) -> DescPairsOutC:
    return out_struct(DESC_PAIRS, ptr, out, rows, node_slots)


def desc_pairs_build(recipe: DescPairsRecipeC, bank: dict, scan_ids: torch.Tensor, seed: int, step: int, pair_base: int,
                     out: dict, workspace: torch.Tensor, rows=None, node_slots=None):
    """f-8: P descriptor pairs with Philox draws (usip_desc_pairs_build_f32) into `out` (DESC_PAIRS_KEYS -> tensors).
    bank: rows, offsets, poses, seq_of, seq_start (device tensors), seq_start_host (int32 numpy), min_rows."""
    return cloud_batch(DESC_PAIRS, recipe, bank, scan_ids, out, workspace, rows, node_slots, counter=(seed, step, pair_base))


def desc_pairs_apply(recipe: DescPairsRecipeC, draws: dict, bank: dict, scan_ids: torch.Tensor, out: dict,
                     workspace: torch.Tensor, rows=None, node_slots=None):
    """f-8 with explicit draws (usip_desc_pairs_apply_f32): DESC_PAIRS_DRAWS -> device tensors in the layouts of
    include/usip_hip.h; tries is i32 [P][T]."""
    return cloud_batch(DESC_PAIRS, recipe, bank, scan_ids, out, workspace, rows, node_slots, draws=draws)


def desc_pairs_workspace_offset(recipe: DescPairsRecipeC, P: int, part: int) -> int:
    """Byte offset of workspace part 0 tables, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud scan ids, 5 total."""
    return cloud_batch_workspace(DESC_PAIRS, recipe, P, part)


def desc_pairs_workspace_bytes(recipe: DescPairsRecipeC, P: int) -> int:
    return cloud_batch_workspace(DESC_PAIRS, recipe, P)


# ---- f-26 indoor descriptor batches (SceneNN): include/usip_hip_indoor_pairs.h, which usip_hip.h includes (_lib keeps
# an included header's structs apart).  The draws struct is f-5's whole: rows, cand, first and params are read and may
# not be absent (INDOOR_PAIRS_DRAWS); the three jitters are not read, may be absent, and are declared so that every
# pointer of the nested struct has a draw that fills it
IndoorPairsRecipeC = _lib.STRUCTS_INCLUDED["usip_indoor_pairs_recipe"]
IndoorPairsBankC = _lib.STRUCTS_INCLUDED["usip_indoor_pairs_bank"]
IndoorPairsDrawsC = _lib.STRUCTS_INCLUDED["usip_indoor_pairs_draws"]
IndoorPairsOutC = _lib.STRUCTS_INCLUDED["usip_indoor_pairs_out"]

INDOOR_PAIRS_KEYS = ("anc_pc", "anc_sn", "anc_node", "pos_pc", "pos_sn", "pos_node", "anc_R_pos", "anc_scale_pos",
                     "anc_shift_pos")
INDOOR_PAIRS_DRAWS = dict(rows=torch.int32, cand=torch.int32, first=torch.int32, params=torch.float64)


@_table
def _indoor_pairs_table(N: int, M: int, Cs: int, P: int) -> dict:
    f = torch.float32
    return dict(_cloud_table(N, M, Cs, P, "anc_", "pos_"), anc_R_pos=((P, 3, 3), f), anc_scale_pos=((P, 1), f),
                anc_shift_pos=((P, 3, 1), f))


def indoor_pairs_shapes(recipe: IndoorPairsRecipeC, P: int) -> dict:
    """key -> shape of one batch of P pairs (all float32): what IndoorDescriptorStep.step documents."""
    return _shapes(INDOOR_PAIRS, recipe, P)


def _indoor_pairs_bank(b: IndoorPairsBankC, bank: dict):
    """bank: rows, offsets, pairs, icp, sample_mode (tensors; the host twin: sample_mode or None), pairs_host (int32
    numpy), min_rows."""
    S, host, modes = bank["pairs"].shape[0], bank["pairs_host"], bank["sample_mode"]
    if tuple(bank["pairs"].shape) != (S, 2) or tuple(bank["icp"].shape) != (S, 12) or host.dtype != "int32" or \
            (modes is not None and tuple(modes.shape) != (S,)) or host.shape != (S, 2) or not host.flags.c_contiguous:
        raise RuntimeError("indoor_pairs: pairs i32 (S, 2), icp f64 (S, 12), sample_mode i32 (S,) on the device and pairs "
                           "as a C-contiguous int32 numpy array")
    b.pairs_host, b.num_frames, b.num_samples = host.ctypes.data, bank["offsets"].shape[0] - 1, S


INDOOR_PAIRS = CloudBatchSpec(
    ids="sample", tag="indoor_pairs", out_c=IndoorPairsOutC, bank_c=IndoorPairsBankC, draws_c=IndoorPairsDrawsC,
    bank=dict(_ROWS, pairs=torch.int32, icp=torch.float64, sample_mode=torch.int32), bank_meta=_indoor_pairs_bank,
    lead=_struct_lead, keys=INDOOR_PAIRS_KEYS,
    out_fields=_out_fields(INDOOR_PAIRS_KEYS, ("anc", "pos"),
                           dict(anc_R_pos="R", anc_scale_pos="scale", anc_shift_pos="shift")),
    table=_indoor_pairs_table, draws=_F5_DRAWS, draw_fields=_draw_fields(cloud=_F5_DRAWS),
    draw_shapes=_f5_draw_shapes, required=tuple(INDOOR_PAIRS_DRAWS),
    index_lead=lambda P: (2, P), clouds=2.0)


def indoor_pairs_out_struct(ptr, out: dict, rows, node_slots) -> IndoorPairsOutC:
    return out_struct(INDOOR_PAIRS, ptr, out, rows, node_slots)


def indoor_pairs_build(recipe: IndoorPairsRecipeC, bank: dict, sample_ids: torch.Tensor, seed: int, step: int,
                       pair_base: int, out: dict, workspace: torch.Tensor, rows=None, node_slots=None):
    """f-26: P indoor descriptor pairs with Philox draws (usip_indoor_pairs_build_f32) into `out` (INDOOR_PAIRS_KEYS).
    bank: rows, offsets, pairs, icp, sample_mode (device tensors), pairs_host (int32 numpy), min_rows."""
    return cloud_batch(INDOOR_PAIRS, recipe, bank, sample_ids, out, workspace, rows, node_slots,
                       counter=(seed, step, pair_base))


def indoor_pairs_apply(recipe: IndoorPairsRecipeC, draws: dict, bank: dict, sample_ids: torch.Tensor, out: dict,
                       workspace: torch.Tensor, rows=None, node_slots=None):
    """f-26 with explicit draws (usip_indoor_pairs_apply_f32): INDOOR_PAIRS_DRAWS -> device tensors in f-5's layouts."""
    return cloud_batch(INDOOR_PAIRS, recipe, bank, sample_ids, out, workspace, rows, node_slots, draws=draws)


def indoor_pairs_workspace_offset(recipe: IndoorPairsRecipeC, P: int, part: int) -> int:
    """Byte offset of workspace part 0 tables, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud frame ids, 5 total."""
    return cloud_batch_workspace(INDOOR_PAIRS, recipe, P, part)


def indoor_pairs_workspace_bytes(recipe: IndoorPairsRecipeC, P: int) -> int:
    return cloud_batch_workspace(INDOOR_PAIRS, recipe, P)


# ---- f-27 evaluation batches from fragments: include/usip_hip_fragment_batch.h; the recipe is f-5's PairsRecipeC, one
# cloud per id, no pair_base, and the ids' host copy (range-checked by the library) rides along
_FRAGMENT_BATCH_STRUCTS = _lib.INCLUDED["usip_hip_fragment_batch.h"][0]
FragmentBatchBankC = _FRAGMENT_BATCH_STRUCTS["usip_fragment_batch_bank"]
FragmentBatchDrawsC = _FRAGMENT_BATCH_STRUCTS["usip_fragment_batch_draws"]
FragmentBatchOutC = _FRAGMENT_BATCH_STRUCTS["usip_fragment_batch_out"]

FRAGMENT_BATCH_KEYS = ("pc", "sn", "node")
FRAGMENT_BATCH_DRAWS = ("rows", "cand", "first")


def fragment_batch_clouds(B: int) -> int:
    """The clouds every buffer of a call of B fragments holds: the cloud stage works in two halves."""
    return 2 * ((int(B) + 1) // 2)


@_table
def _fragment_batch_table(N: int, M: int, Cs: int, B: int) -> dict:
    return _cloud_table(N, M, Cs, fragment_batch_clouds(B), "")


def fragment_batch_shapes(recipe: PairsRecipeC, B: int) -> dict:
    """key -> shape of the buffers of one call of B fragments (float32): B2 = fragment_batch_clouds(B) clouds each."""
    return _shapes(FRAGMENT_BATCH, recipe, B)


def _fragment_batch_bank(b: FragmentBatchBankC, bank: dict):
    b.num_fragments = bank["offsets"].shape[0] - 1


def _fragment_batch_lead(ptr, bank, b, ids, B, ids_host, on_device) -> tuple:
    return (ctypes.addressof(b), ids) + ((ids_host,) if on_device else ()) + (B,)


FRAGMENT_BATCH = CloudBatchSpec(
    ids="fragment", tag="fragment_batch", out_c=FragmentBatchOutC, bank_c=FragmentBatchBankC,
    draws_c=FragmentBatchDrawsC, bank=_ROWS, bank_meta=_fragment_batch_bank, lead=_fragment_batch_lead,
    keys=FRAGMENT_BATCH_KEYS, out_fields=_out_fields(FRAGMENT_BATCH_KEYS), table=_fragment_batch_table,
    draws=dict.fromkeys(FRAGMENT_BATCH_DRAWS, torch.int32), draw_fields=_draw_fields(own=FRAGMENT_BATCH_DRAWS),
    draw_shapes=lambda c, B: dict(rows=(B, c.N), cand=(B, c.n_sub), first=(B,)), required=FRAGMENT_BATCH_DRAWS,
    index_lead=lambda B: (fragment_batch_clouds(B),), clouds=1.0)


def fragment_batch_out_struct(ptr, out: dict, rows, node_slots) -> FragmentBatchOutC:
    return out_struct(FRAGMENT_BATCH, ptr, out, rows, node_slots)


def fragment_batch_build(recipe: PairsRecipeC, bank: dict, ids: torch.Tensor, ids_host, seed: int, step: int, out: dict,
                         workspace: torch.Tensor, rows=None, node_slots=None):
    """f-27: B evaluation fragments with Philox draws (usip_fragment_batch_build_f32) into `out` (FRAGMENT_BATCH_KEYS, each
    holding fragment_batch_clouds(B) clouds).  bank: rows, offsets (device tensors), min_rows; ids_host: the ids as an
    int32 numpy array (range-checked by the library) or None."""
    return cloud_batch(FRAGMENT_BATCH, recipe, bank, ids, out, workspace, rows, node_slots, counter=(seed, step),
                       ids_host=ids_host)


def fragment_batch_apply(recipe: PairsRecipeC, draws: dict, bank: dict, ids: torch.Tensor, ids_host, out: dict,
                         workspace: torch.Tensor, rows=None, node_slots=None):
    """f-27 with explicit draws (usip_fragment_batch_apply_f32): rows i32 (B, N), cand i32 (B, n_sub), first i32 (B,)."""
    return cloud_batch(FRAGMENT_BATCH, recipe, bank, ids, out, workspace, rows, node_slots, draws=draws, ids_host=ids_host)


def fragment_batch_workspace_offset(recipe: PairsRecipeC, B: int, part: int) -> int:
    """Byte offset of workspace part 0 table, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud fragment ids, 5 total."""
    return cloud_batch_workspace(FRAGMENT_BATCH, recipe, B, part)


def fragment_batch_workspace_bytes(recipe: PairsRecipeC, B: int) -> int:
    return cloud_batch_workspace(FRAGMENT_BATCH, recipe, B)


# ------------------------------------------------------------------------------------------------ f-6 evaluation
def _opt_ptr(t):
    return _ptr(t) if t is not None else None


def _need_pairs(x1, x2, count, limit):
    _need(x1, "x1", torch.float32)
    _need(x2, "x2", torch.float32)
    _need(count, "count", torch.int32)
    if x1.dim() != 3 or x1.shape[1] != 3 or x2.shape != x1.shape or count.shape != (x1.shape[0],):
        raise RuntimeError("registration: expected x1, x2 f32 [P,3,Nmax] and count i32 [P]")
    if not 1 <= x1.shape[2] <= limit:
        raise RuntimeError("registration: Nmax must be in 1..%d (got %d)" % (limit, x1.shape[2]))
    return x1.shape[0], x1.shape[2]


def _need_on(t, name, dtype, shape, device):
    if t is None:
        return
    _need(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise RuntimeError("registration: %s must be %s %s on %s" % (name, dtype, tuple(shape), device))


RANSAC_NMAX, RANSAC_NMAX_LARGE = 1024, 10240      # the outdoor evaluation's keypoints per frame; the library's limit


def ransac_trials(x1, x2, count, T: int, threshold: float, seed: int = 0, pair_ids=None, triplets=None,
                  want_hypotheses: bool = False, want_triplets: bool = False, _nmax: int = RANSAC_NMAX):
    """f-6: inlier counts of T rigid-fit trials per pair -> (counts i32 [P,T], hypotheses f64 [P,T,3,4] or None, drawn
    triplets i32 [P,T,3] or None).  triplets i32 [P,T,3]: explicit draws; otherwise Philox draws of (seed, pair_ids).
    Nmax <= 1024; ransac_trials_large (f-9) is the same call with Nmax <= 10240."""
    P, Nmax = _need_pairs(x1, x2, count, _nmax)
    T = int(T)
    dev = x1.device
    _need_on(pair_ids, "pair_ids", torch.int64, (P,), dev)
    _need_on(triplets, "triplets", torch.int32, (P, T, 3), dev)
    counts = torch.empty((P, T), dtype=torch.int32, device=dev)
    hyp = torch.empty((P, T, 3, 4), dtype=torch.float64, device=dev) if want_hypotheses else None
    drawn = torch.empty((P, T, 3), dtype=torch.int32, device=dev) if want_triplets and triplets is None else triplets
    with torch.cuda.device(dev), prof.kernel("ransac_trials", 24.0 * P * Nmax + 4.0 * P * T, 30.0 * P * T * Nmax):
        if triplets is None:
            _lib.check(_lib.lib().usip_ransac_trials_f32(
                _ptr(x1), _ptr(x2), _ptr(count), P, Nmax, T, float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF,
                _opt_ptr(pair_ids), _ptr(counts), _opt_ptr(hyp), _opt_ptr(drawn), _stream(x1)), "usip_ransac_trials_f32")
        else:
            _lib.check(_lib.lib().usip_ransac_trials_explicit_f32(
                _ptr(x1), _ptr(x2), _ptr(count), P, Nmax, T, float(threshold), _ptr(triplets), _ptr(counts),
                _opt_ptr(hyp), _stream(x1)), "usip_ransac_trials_explicit_f32")
    return counts, hyp, (drawn if want_triplets else None)


def ransac_select(x1, x2, count, counts, max_trials: int, threshold: float, seed: int = 0, pair_ids=None, triplets=None,
                  gt=None, _nmax: int = RANSAC_NMAX):
    """f-6: ransac.m's stopping rule replayed over counts i32 [P,T], the chosen hypothesis' inliers and the refit ->
    dict(Rt f64 [P,3,4], inlier_mask u8 [P,Nmax], inliers, trialcount, chosen i32 [P], valid u8 [P], delta_t, delta_deg
    f64 [P] or None without gt).  Nmax <= 1024; ransac_select_large (f-9) is the same call with Nmax <= 10240."""
    P, Nmax = _need_pairs(x1, x2, count, _nmax)
    dev = x1.device
    _need(counts, "counts", torch.int32)
    if counts.dim() != 2 or counts.shape[0] != P or counts.device != dev:
        raise RuntimeError("registration: counts must be i32 [P,T] on %s" % dev)
    T = counts.shape[1]
    if not 0 <= int(max_trials) <= T - 1:
        raise RuntimeError("registration: max_trials must be in 0..T-1 (T = %d, got %d)" % (T, max_trials))
    _need_on(pair_ids, "pair_ids", torch.int64, (P,), dev)
    _need_on(triplets, "triplets", torch.int32, (P, T, 3), dev)
    _need_on(gt, "gt", torch.float64, (P, 3, 4), dev)
    out = {"Rt": torch.empty((P, 3, 4), dtype=torch.float64, device=dev),
           "inlier_mask": torch.empty((P, Nmax), dtype=torch.uint8, device=dev),
           "inliers": torch.empty((P,), dtype=torch.int32, device=dev),
           "trialcount": torch.empty((P,), dtype=torch.int32, device=dev),
           "valid": torch.empty((P,), dtype=torch.uint8, device=dev),
           "chosen": torch.empty((P,), dtype=torch.int32, device=dev),
           "delta_t": torch.empty((P,), dtype=torch.float64, device=dev) if gt is not None else None,
           "delta_deg": torch.empty((P,), dtype=torch.float64, device=dev) if gt is not None else None}
    with torch.cuda.device(dev), prof.kernel("ransac_select", 4.0 * P * T + 24.0 * P * Nmax, 60.0 * P * Nmax):
        _lib.check(_lib.lib().usip_ransac_select_f32(
            _ptr(x1), _ptr(x2), _ptr(count), P, Nmax, T, int(max_trials), float(threshold),
            int(seed) & 0xFFFFFFFFFFFFFFFF, _opt_ptr(pair_ids), _opt_ptr(triplets), _ptr(counts), _opt_ptr(gt),
            _ptr(out["Rt"]), _ptr(out["inlier_mask"]), _ptr(out["inliers"]), _ptr(out["trialcount"]), _ptr(out["valid"]),
            _ptr(out["chosen"]), _opt_ptr(out["delta_t"]), _opt_ptr(out["delta_deg"]), _stream(x1)),
            "usip_ransac_select_f32")
    return out


def compare_transform(gt, Rt):
    """f-6: Utils.compareTransform on gt, Rt f64 [P,3,4] -> (delta_t, delta_deg) f64 [P]."""
    _need(gt, "gt", torch.float64)
    _need(Rt, "Rt", torch.float64)
    if gt.dim() != 3 or tuple(gt.shape[1:]) != (3, 4) or Rt.shape != gt.shape or Rt.device != gt.device:
        raise RuntimeError("compare_transform: expected gt, Rt f64 [P,3,4] on one device")
    P = gt.shape[0]
    dt = torch.empty((P,), dtype=torch.float64, device=gt.device)
    dd = torch.empty((P,), dtype=torch.float64, device=gt.device)
    with torch.cuda.device(gt.device), prof.kernel("compare_transform", 208.0 * P):
        _lib.check(_lib.lib().usip_compare_transform_f64(_ptr(gt), _ptr(Rt), P, _ptr(dt), _ptr(dd), _stream(gt)),
                   "usip_compare_transform_f64")
    return dt, dd


def repeatability(anc, anc_count, pos, pos_count, gt, radius: float):
    """f-6: eval_rep.m on ragged batches: anc f32 [P,3,Ma], pos f32 [P,3,Mp], counts i32 [P], gt f64 [P,3,4] ->
    (min_dist f64 [P,Ma], hits i32 [P], ratio f64 [P])."""
    _need_pts(anc, "anc")
    _need_pts(pos, "pos")
    P, _, Ma = anc.shape
    Mp = pos.shape[2]
    dev = anc.device
    if pos.shape[0] != P or pos.device != dev or Ma < 1 or Mp < 1:
        raise RuntimeError("repeatability: expected anc [P,3,Ma], pos [P,3,Mp] on one device")
    _need_on(anc_count, "anc_count", torch.int32, (P,), dev)
    _need_on(pos_count, "pos_count", torch.int32, (P,), dev)
    _need_on(gt, "gt", torch.float64, (P, 3, 4), dev)
    if anc_count is None or pos_count is None or gt is None:
        raise RuntimeError("repeatability: anc_count, pos_count and gt are required")
    md = torch.empty((P, Ma), dtype=torch.float64, device=dev)
    hits = torch.empty((P,), dtype=torch.int32, device=dev)
    ratio = torch.empty((P,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), prof.kernel("repeatability", 12.0 * P * (Ma + Mp), 8.0 * P * Ma * Mp):
        _lib.check(_lib.lib().usip_repeatability_f32(_ptr(anc), _ptr(anc_count), _ptr(pos), _ptr(pos_count), _ptr(gt),
                                                     float(radius), P, Ma, Mp, _ptr(md), _ptr(hits), _ptr(ratio),
                                                     _stream(anc)), "usip_repeatability_f32")
    return md, hits, ratio


def nearest_nd_counted(a, b, a_count, b_count):
    """f-6: nearest_nd with per-frame counts: a f32 [B,C,Ma], b f32 [B,C,Nb], counts i32 [B] -> (min distance f32 [B,Ma],
    first arg-min i32 [B,Ma]); rows beyond a_count get (inf, 0)."""
    _need(a, "a", torch.float32)
    _need(b, "b", torch.float32)
    if a.dim() != 3 or b.dim() != 3 or a.shape[:2] != b.shape[:2] or a.device != b.device or b.shape[2] < 1:
        raise RuntimeError("nearest_nd_counted: expected a [B,C,Ma] and b [B,C,Nb] on one device")
    B, C, Ma = a.shape
    Nb = b.shape[2]
    _need_on(a_count, "a_count", torch.int32, (B,), a.device)
    _need_on(b_count, "b_count", torch.int32, (B,), a.device)
    if a_count is None or b_count is None:
        raise RuntimeError("nearest_nd_counted: counts are required")
    d = torch.empty((B, Ma), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, Ma), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device), prof.kernel("nearest_nd_counted", 4.0 * B * C * (Ma + Nb), 3.0 * B * C * Ma * Nb):
        _lib.check(_lib.lib().usip_nearest_nd_counted_f32(_ptr(a), _ptr(b), _ptr(a_count), _ptr(b_count), _ptr(d),
                                                          _ptr(arg), B, C, Ma, Nb, _stream(a)),
                   "usip_nearest_nd_counted_f32")
    return d, arg


# ------------------------------------------------------------------------------------------------ f-7 scan preparation
def _need_scan(xyzi, K=None):
    _need(xyzi, "xyzi", torch.float32)
    if xyzi.dim() != 2 or xyzi.shape[1] != 4:
        raise RuntimeError("prepare: expected xyzi f32 [n,4] (x y z reflectance)")
    n = xyzi.shape[0]
    if not 1 <= n <= 1 << 20:
        raise RuntimeError("prepare: n must be in 1..2^20 (got %d)" % n)
    if K is not None and not (1 <= int(K) <= 16 and n >= int(K) + 1):
        raise RuntimeError("prepare: K must be in 1..16 and n >= K + 1 (got K = %d, n = %d)" % (K, n))
    return n


def scan_knn(xyzi, perm, K: int, want_visits: bool = False):
    """f-7: xyzi f32 [n,4], perm i32 [n] (the order of the points along x) -> idx i32 [n,K]: the K nearest OTHER points of
    every point, ascending (d2, index); with want_visits also the 256-point tiles each workgroup walked, i32 [ceil(n/256)]."""
    K = int(K)
    n = _need_scan(xyzi, K)
    _need_on(perm, "perm", torch.int32, (n,), xyzi.device)
    idx = torch.empty((n, K), dtype=torch.int32, device=xyzi.device)
    visits = torch.empty(((n + 255) // 256,), dtype=torch.int32, device=xyzi.device) if want_visits else None
    with torch.cuda.device(xyzi.device), prof.kernel("scan_knn", 16.0 * n + 4.0 * n * K, keyed=True):
        _lib.check(_lib.lib().usip_scan_knn_f32(_ptr(xyzi), _ptr(perm), n, K, _ptr(idx), _opt_ptr(visits), _stream(xyzi)),
                   "usip_scan_knn_f32")
    return (idx, visits) if want_visits else idx


def scan_normals(xyzi, idx, viewpoint=(0.0, 0.0, 1.0)):
    """f-7: xyzi f32 [n,4], idx i32 [n,K] -> (f64 [n,4], f32 [n,4]): nx ny nz curvature, flipped towards `viewpoint`."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2:
        raise RuntimeError("prepare: idx must be i32 [n,K]")
    K = idx.shape[1]
    n = _need_scan(xyzi, K)
    _need_on(idx, "idx", torch.int32, (n, K), xyzi.device)
    view = (ctypes.c_double * 3)(*[float(v) for v in viewpoint])
    n64 = torch.empty((n, 4), dtype=torch.float64, device=xyzi.device)
    n32 = torch.empty((n, 4), dtype=torch.float32, device=xyzi.device)
    with torch.cuda.device(xyzi.device), prof.kernel("scan_normals", (16.0 * (K + 1) + 4.0 * K + 48.0) * n, keyed=True):
        _lib.check(_lib.lib().usip_scan_normals_f32(_ptr(xyzi), _ptr(idx), n, K, ctypes.addressof(view), _ptr(n64),
                                                    _ptr(n32), _stream(xyzi)), "usip_scan_normals_f32")
    return n64, n32


def scan_voxel_keys(xyzi, lohi, leaf: float):
    """f-7: xyzi f32 [n,4], lohi f32 [6] (per-axis minimum, then maximum, on the device) -> keys i64 [n]."""
    n = _need_scan(xyzi)
    _need_on(lohi, "lohi", torch.float32, (6,), xyzi.device)
    if not float(leaf) > 0.0:
        raise RuntimeError("prepare: leaf must be positive")
    keys = torch.empty((n,), dtype=torch.int64, device=xyzi.device)
    with torch.cuda.device(xyzi.device), prof.kernel("scan_voxel_keys", 24.0 * n, keyed=True):
        _lib.check(_lib.lib().usip_scan_voxel_keys_f32(_ptr(xyzi), n, _ptr(lohi), float(leaf), _ptr(keys), _stream(xyzi)),
                   "usip_scan_voxel_keys_f32")
    return keys


def scan_voxel_average(xyzi, normals_f64, perm, start):
    """f-7: the members perm[start[c] : start[c + 1]] of every occupied cell c averaged -> rows f32 [m,8]."""
    n = _need_scan(xyzi)
    dev = xyzi.device
    _need_on(normals_f64, "normals_f64", torch.float64, (n, 4), dev)
    _need_on(perm, "perm", torch.int32, (n,), dev)
    _need(start, "start", torch.int32)
    if start.dim() != 1 or start.device != dev or not 1 <= start.shape[0] <= n + 1:
        raise RuntimeError("prepare: start must be i32 [m + 1] on %s with m <= n" % dev)
    m = start.shape[0] - 1
    rows = torch.empty((m, 8), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), prof.kernel("scan_voxel_average", 52.0 * n + 36.0 * m, keyed=True):
        _lib.check(_lib.lib().usip_scan_voxel_average_f32(_ptr(xyzi), _ptr(normals_f64), _ptr(perm), _ptr(start), n, m,
                                                          _ptr(rows), _stream(xyzi)), "usip_scan_voxel_average_f32")
    return rows


# ------------------------------------------------------------------------------------------------ f-9 fragment registration
def knn_nd_counted(a, b, a_count, b_count, k: int):
    """f-9: the k nearest rows of b for every row of a on ragged batches: a f32 [B,C,Ma], b f32 [B,C,Nb], counts i32 [B]
    -> (dist f32 [B,Ma,k], idx i32 [B,Ma,k] ascending, lower index on ties; valid i32 [B] = min(k, b_count) columns)."""
    _need(a, "a", torch.float32)
    _need(b, "b", torch.float32)
    if a.dim() != 3 or b.dim() != 3 or a.shape[:2] != b.shape[:2] or a.device != b.device or b.shape[2] < 1:
        raise RuntimeError("knn_nd_counted: expected a [B,C,Ma] and b [B,C,Nb] on one device")
    k = int(k)
    if not 1 <= k <= 8:
        raise RuntimeError("knn_nd_counted: k must be in 1..8 (got %d)" % k)
    B, C, Ma = a.shape
    Nb = b.shape[2]
    _need_on(a_count, "a_count", torch.int32, (B,), a.device)
    _need_on(b_count, "b_count", torch.int32, (B,), a.device)
    if a_count is None or b_count is None:
        raise RuntimeError("knn_nd_counted: counts are required")
    d = torch.empty((B, Ma, k), dtype=torch.float32, device=a.device)
    idx = torch.empty((B, Ma, k), dtype=torch.int32, device=a.device)
    valid = torch.zeros((B,), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device), prof.kernel("knn_nd_counted", 4.0 * B * C * (Ma + Nb), 3.0 * B * C * Ma * Nb):
        _lib.check(_lib.lib().usip_knn_nd_counted_f32(_ptr(a), _ptr(b), _ptr(a_count), _ptr(b_count), k, _ptr(d),
                                                      _ptr(idx), _ptr(valid), B, C, Ma, Nb, _stream(a)),
                   "usip_knn_nd_counted_f32")
    return d, idx, valid


def match_union(nn12, nn21, a_count, p_count):
    """f-9: nn12 i32 [P,Ma,k], nn21 i32 [P,Mp,k], keypoint counts i32 [P] -> (pairs i32 [P,Cmax,2] sorted by (i, q), count
    i32 [P]); Cmax = k (Ma + Mp) <= 10240."""
    _need(nn12, "nn12", torch.int32)
    _need(nn21, "nn21", torch.int32)
    if nn12.dim() != 3 or nn21.dim() != 3 or nn12.shape[0] != nn21.shape[0] or nn12.shape[2] != nn21.shape[2] or \
            nn12.device != nn21.device:
        raise RuntimeError("match_union: expected nn12 [P,Ma,k] and nn21 [P,Mp,k] on one device")
    P, Ma, k = nn12.shape
    Mp = nn21.shape[1]
    Cmax = k * (Ma + Mp)
    if not (1 <= k <= 8 and Ma >= 1 and Mp >= 1 and Cmax <= 10240):
        raise RuntimeError("match_union: k (Ma + Mp) must be at most 10240 with k in 1..8 (got k = %d, Ma = %d, Mp = %d)"
                           % (k, Ma, Mp))
    _need_on(a_count, "a_count", torch.int32, (P,), nn12.device)
    _need_on(p_count, "p_count", torch.int32, (P,), nn12.device)
    if a_count is None or p_count is None:
        raise RuntimeError("match_union: counts are required")
    pairs = torch.empty((P, Cmax, 2), dtype=torch.int32, device=nn12.device)
    count = torch.empty((P,), dtype=torch.int32, device=nn12.device)
    with torch.cuda.device(nn12.device), prof.kernel("match_union", 12.0 * P * Cmax):
        _lib.check(_lib.lib().usip_match_union_i32(_ptr(nn12), _ptr(nn21), _ptr(a_count), _ptr(p_count), P, Ma, Mp, k,
                                                   _ptr(pairs), _ptr(count), _stream(nn12)), "usip_match_union_i32")
    return pairs, count


ransac_trials_large = functools.partial(ransac_trials, _nmax=RANSAC_NMAX_LARGE)      # f-9: up to 10240 correspondences
ransac_select_large = functools.partial(ransac_select, _nmax=RANSAC_NMAX_LARGE)


def information(x, mask):
    """f-9: x f32 [P,3,Nmax], mask u8 [P,Nmax] -> info f64 [P,6,6]: the sum of A'A over the masked points."""
    _need(x, "x", torch.float32)
    _need(mask, "mask", torch.uint8)
    if x.dim() != 3 or x.shape[1] != 3 or tuple(mask.shape) != (x.shape[0], x.shape[2]) or mask.device != x.device or \
            not 1 <= x.shape[2] <= 10240:
        raise RuntimeError("information: expected x f32 [P,3,Nmax] and mask u8 [P,Nmax] on one device, Nmax <= 10240")
    P, _, Nmax = x.shape
    info = torch.empty((P, 6, 6), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device), prof.kernel("information", 13.0 * P * Nmax):
        _lib.check(_lib.lib().usip_information_f32(_ptr(x), _ptr(mask), P, Nmax, _ptr(info), _stream(x)),
                   "usip_information_f32")
    return info


def _need_bank(rows, offsets, frag1, frag2, Rt):
    _need(rows, "rows", torch.float32)
    _need(offsets, "offsets", torch.int64)
    if rows.dim() != 2 or rows.shape[1] < 3 or offsets.dim() != 1 or offsets.shape[0] < 2 or offsets.device != rows.device:
        raise RuntimeError("overlap: expected rows f32 [total,row_len >= 3] and offsets i64 [fragments + 1] on one device")
    P = frag2.shape[0]
    _need_on(frag2, "frag2", torch.int32, (P,), rows.device)
    _need_on(frag1, "frag1", torch.int32, (P,), rows.device)
    _need_on(Rt, "Rt", torch.float64, (P, 3, 4), rows.device)
    return P


def _bank_args(rows, offsets):
    """the C argument run rows, row_len, offsets, num_frags, total_rows of a CSR bank"""
    return _ptr(rows), rows.shape[1], _ptr(offsets), offsets.shape[0] - 1, rows.shape[0]


def overlap_keys(rows, offsets, frag2, Rt, Lmax: int):
    """f-9: x of every fragment-2 point moved by Rt -> keys f64 [P,Lmax] (+inf beyond the fragment), to sort by."""
    P = _need_bank(rows, offsets, None, frag2, Rt)
    keys = torch.empty((P, int(Lmax)), dtype=torch.float64, device=rows.device)
    with torch.cuda.device(rows.device), prof.kernel("overlap_keys", 20.0 * P * Lmax):
        _lib.check(_lib.lib().usip_overlap_keys_f32(*_bank_args(rows, offsets), _ptr(frag2), _ptr(Rt), P, int(Lmax),
                                                    _ptr(keys), _stream(rows)), "usip_overlap_keys_f32")
    return keys


def overlap_ratio(rows, offsets, frag1, frag2, Rt, perm1, perm2, radius: float):
    """f-9: ratioAligned of register2Fragments.m on a CSR bank -> (ratio f64 [P,2], hits i32 [P,2]).  perm1 i32 [total]:
    every fragment's local rows ascending along x; perm2 i32 [P,Lmax]: fragment 2's ascending along overlap_keys."""
    P = _need_bank(rows, offsets, frag1, frag2, Rt)
    _need_on(perm1, "perm1", torch.int32, (rows.shape[0],), rows.device)
    _need(perm2, "perm2", torch.int32)
    if perm2.dim() != 2 or perm2.shape[0] != P or perm2.device != rows.device or perm2.shape[1] < 1:
        raise RuntimeError("overlap: perm2 must be i32 [P,Lmax] on %s" % rows.device)
    Lmax = perm2.shape[1]
    hits = torch.empty((P, 2), dtype=torch.int32, device=rows.device)
    ratio = torch.empty((P, 2), dtype=torch.float64, device=rows.device)
    with torch.cuda.device(rows.device), prof.kernel("overlap_ratio", 32.0 * P * Lmax):
        _lib.check(_lib.lib().usip_overlap_ratio_f32(*_bank_args(rows, offsets), _ptr(frag1), _ptr(frag2), _ptr(Rt),
                                                     _ptr(perm1), _ptr(perm2), P, Lmax, float(radius), _ptr(hits),
                                                     _ptr(ratio), _stream(rows)), "usip_overlap_ratio_f32")
    return ratio, hits


# ------------------------------------------------------------------------------------------------ f-11 baseline keypoints
def _need_frames(pc, count, perm=None, tag="iss"):
    """pc f32 [B,3,N] with count i32 [B] or None and, where the kernel walks a sorted frame, perm i32 [B,N] (a missing one is
    the library's to refuse) -> (B, N)"""
    _need(pc, "pc", torch.float32)
    if pc.dim() != 3 or pc.shape[1] != 3:
        raise RuntimeError("%s: expected pc f32 [B,3,N]" % tag)
    B, _, N = pc.shape
    if not (1 <= N <= 1 << 20 and 1 <= B <= 65535):
        raise RuntimeError("%s: N must be in 1..2^20 and B in 1..65535 (got B = %d, N = %d)" % (tag, B, N))
    _need_on(count, "count", torch.int32, (B,), pc.device)
    _need_on(perm, "perm", torch.int32, (B, N), pc.device)
    return B, N


def _visits(B, N, device, want):
    """tiles_visited i32 [B, ceil(N/256)] for a kernel to fill, or None"""
    return torch.empty((B, (N + 255) // 256), dtype=torch.int32, device=device) if want else None


def iss_saliency(pc, count, perm, salient_radius: float, gamma_21: float, gamma_32: float, min_neighbors: int,
                 want_visits: bool = False):
    """f-11: pc f32 [B,3,N], count i32 [B] or None, perm i32 [B,N] (every frame's live points ascending along x, stable)
    -> (saliency f64 [B,N], neighbours i32 [B,N]); with want_visits also the 256-point tiles each workgroup walked, i32
    [B, ceil(N/256)]."""
    B, N = _need_frames(pc, count, perm)
    if not (float(salient_radius) > 0.0 and int(min_neighbors) >= 1):
        raise RuntimeError("iss: salient_radius must be positive and min_neighbors at least 1")
    sal = torch.empty((B, N), dtype=torch.float64, device=pc.device)
    nb = torch.empty((B, N), dtype=torch.int32, device=pc.device)
    visits = _visits(B, N, pc.device, want_visits)
    with torch.cuda.device(pc.device), prof.kernel("iss_saliency", 28.0 * B * N, keyed=True):
        _lib.check(_lib.lib().usip_iss_saliency_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), B, N, float(salient_radius),
                                                    float(gamma_21), float(gamma_32), int(min_neighbors), _ptr(sal),
                                                    _ptr(nb), _opt_ptr(visits), _stream(pc)), "usip_iss_saliency_f32")
    return (sal, nb, visits) if want_visits else (sal, nb)


def iss_nms(pc, count, perm, saliency, non_max_radius: float, min_neighbors: int):
    """f-11: saliency f64 [B,N] -> keypoint u8 [B,N]: salient, enough neighbours within non_max_radius, none of them larger."""
    B, N = _need_frames(pc, count, perm)
    _need_on(saliency, "saliency", torch.float64, (B, N), pc.device)
    if saliency is None or not (float(non_max_radius) > 0.0 and int(min_neighbors) >= 1):
        raise RuntimeError("iss: saliency is required, non_max_radius must be positive and min_neighbors at least 1")
    kp = torch.empty((B, N), dtype=torch.uint8, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("iss_nms", 25.0 * B * N, keyed=True):
        _lib.check(_lib.lib().usip_iss_nms_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _ptr(saliency), B, N,
                                               float(non_max_radius), int(min_neighbors), _ptr(kp), _stream(pc)),
                   "usip_iss_nms_f32")
    return kp


# ------------------------------------------------------------------------------------------------ f-16 baseline keypoints: Harris3D
HARRIS_METHODS = {"harris": 0, "noble": 1, "lowe": 2, "tomasi": 3}


def harris_normals(pc, count, perm, radius: float, min_neighbors: int = 3):
    """f-16: pc f32 [B,3,N], count i32 [B] or None, perm i32 [B,N] (every frame's live points ascending along x, stable)
    -> (normals f64 [B,3,N], neighbours i32 [B,N]); a point with fewer than min_neighbors members within radius has no
    normal: zeros."""
    B, N = _need_frames(pc, count, perm, "harris")
    if not (float(radius) > 0.0 and int(min_neighbors) >= 1):
        raise RuntimeError("harris: radius must be positive and min_neighbors at least 1")
    normals = torch.empty((B, 3, N), dtype=torch.float64, device=pc.device)
    nb = torch.empty((B, N), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("harris_normals", 40.0 * B * N, keyed=True):
        _lib.check(_lib.lib().usip_harris_normals_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), B, N, float(radius),
                                                      int(min_neighbors), _ptr(normals), _ptr(nb), _stream(pc)),
                   "usip_harris_normals_f32")
    return normals, nb


def harris_response(pc, count, perm, normals, radius: float, response: str = "harris", want_visits: bool = False):
    """f-16: normals f64 [B,3,N] (a row that is not finite or all zero: no normal) -> (response f64 [B,N], members i32
    [B,N]); with want_visits also the 256-point tiles each workgroup walked, i32 [B, ceil(N/256)]."""
    B, N = _need_frames(pc, count, perm, "harris")
    _need_on(normals, "normals", torch.float64, (B, 3, N), pc.device)
    if normals is None or not float(radius) > 0.0:
        raise RuntimeError("harris: normals are required and radius must be positive")
    if response not in HARRIS_METHODS:
        raise RuntimeError("harris: response must be one of %s, got %r" % (sorted(HARRIS_METHODS), response))
    res = torch.empty((B, N), dtype=torch.float64, device=pc.device)
    members = torch.empty((B, N), dtype=torch.int32, device=pc.device)
    visits = _visits(B, N, pc.device, want_visits)
    with torch.cuda.device(pc.device), prof.kernel("harris_response", 64.0 * B * N, keyed=True):
        _lib.check(_lib.lib().usip_harris_response_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _ptr(normals), B, N,
                                                       float(radius), HARRIS_METHODS[response], _ptr(res), _ptr(members),
                                                       _opt_ptr(visits), _stream(pc)), "usip_harris_response_f32")
    return (res, members, visits) if want_visits else (res, members)


# ------------------------------------------------------------------------------------------------ f-19 baseline descriptor: FPFH
FPFH_WIDTH, FPFH_MMAX = 33, 65535


def fpfh_spfh(pc, count, perm, normals, radius: float, want_visits: bool = False):
    """f-19: normals f64 [B,3,N] (a row that is not finite or all zero: no normal) -> (spfh i32 [B,N,33], the integer counts of
    the three 11-bin pair-feature histograms over every point's members, members i32 [B,N]); with want_visits also the
    256-point tiles each workgroup walked, i32 [B, ceil(N/256)]."""
    B, N = _need_frames(pc, count, perm, "fpfh")
    _need_on(normals, "normals", torch.float64, (B, 3, N), pc.device)
    if normals is None or not float(radius) > 0.0:
        raise RuntimeError("fpfh: normals are required and radius must be positive")
    spfh = torch.empty((B, N, FPFH_WIDTH), dtype=torch.int32, device=pc.device)
    members = torch.empty((B, N), dtype=torch.int32, device=pc.device)
    visits = _visits(B, N, pc.device, want_visits)
    with torch.cuda.device(pc.device), prof.kernel("fpfh_spfh", (40.0 + 4.0 * FPFH_WIDTH) * B * N, keyed=True):
        _lib.check(_lib.lib().usip_fpfh_spfh_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _ptr(normals), B, N, float(radius),
                                                 _ptr(spfh), _ptr(members), _opt_ptr(visits), _stream(pc)),
                   "usip_fpfh_spfh_f32")
    return (spfh, members, visits) if want_visits else (spfh, members)


def fpfh_gather(pc, count, perm, spfh, members, keypoints, kp_count, radius: float):
    """f-19: keypoints f32 [B,3,M] (any positions), kp_count i32 [B] or None -> (fpfh f64 [B,M,33], kp_members i32 [B,M]): the
    SPFH rows of the cloud points within the radius of each keypoint, weighted by 1 / squared distance, each block of eleven
    scaled to the sum 100."""
    B, N = _need_frames(pc, count, perm, "fpfh")
    M = _need_keypoints(pc, keypoints, kp_count, "fpfh")
    _need_on(spfh, "spfh", torch.int32, (B, N, FPFH_WIDTH), pc.device)
    _need_on(members, "members", torch.int32, (B, N), pc.device)
    if spfh is None or members is None or not float(radius) > 0.0:
        raise RuntimeError("fpfh: spfh and members are required and radius must be positive")
    fpfh = torch.empty((B, M, FPFH_WIDTH), dtype=torch.float64, device=pc.device)
    kp_members = torch.empty((B, M), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("fpfh_gather", 16.0 * B * N + (8.0 * FPFH_WIDTH + 16.0) * B * M, keyed=True):
        _lib.check(_lib.lib().usip_fpfh_gather_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _ptr(spfh), _ptr(members),
                                                   _ptr(keypoints), _opt_ptr(kp_count), B, N, M, float(radius), _ptr(fpfh),
                                                   _ptr(kp_members), _stream(pc)), "usip_fpfh_gather_f32")
    return fpfh, kp_members


# ------------------------------------------------------------------------------------------------ f-20 baseline descriptor: SHOT
SHOT_WIDTH = 352


def _need_keypoints(pc, keypoints, kp_count, tag):
    """keypoints f32 [B,3,M] beside pc f32 [B,3,N], kp_count i32 [B] or None -> M"""
    _need(keypoints, "keypoints", torch.float32)
    if keypoints.dim() != 3 or keypoints.shape[0] != pc.shape[0] or keypoints.shape[1] != 3 or keypoints.device != pc.device \
            or not 1 <= keypoints.shape[2] <= FPFH_MMAX:
        raise RuntimeError("%s: expected keypoints f32 [B,3,M] on %s with M in 1..%d" % (tag, pc.device, FPFH_MMAX))
    _need_on(kp_count, "kp_count", torch.int32, (pc.shape[0],), pc.device)
    return keypoints.shape[2]


def _histogram_rows(B, M, width, device):
    """(hist i64, desc f64, both [B,M,width], kp_members i32 [B,M]) for a histogram kernel to fill"""
    return (torch.empty((B, M, width), dtype=torch.int64, device=device),
            torch.empty((B, M, width), dtype=torch.float64, device=device),
            torch.empty((B, M), dtype=torch.int32, device=device))


def shot_lrf(pc, count, perm, keypoints, kp_count, radius: float):
    """f-20: keypoints f32 [B,3,M] (any positions), kp_count i32 [B] or None -> (lrf f64 [B,M,9], the rows x, y, z of every
    keypoint's local reference frame over the live points within the radius, zeros where there is none; lrf_members i32
    [B,M])."""
    B, N = _need_frames(pc, count, perm, "shot")
    M = _need_keypoints(pc, keypoints, kp_count, "shot")
    if not float(radius) > 0.0:
        raise RuntimeError("shot: radius must be positive")
    lrf = torch.empty((B, M, 9), dtype=torch.float64, device=pc.device)
    members = torch.empty((B, M), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("shot_lrf", 16.0 * B * N + 88.0 * B * M, keyed=True):
        _lib.check(_lib.lib().usip_shot_lrf_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _ptr(keypoints), _opt_ptr(kp_count),
                                                B, N, M, float(radius), _ptr(lrf), _ptr(members), _stream(pc)),
                   "usip_shot_lrf_f32")
    return lrf, members


def shot_hist(pc, count, perm, normals, keypoints, kp_count, lrf, radius: float):
    """f-20: normals f64 [B,3,N] (a row that is not finite or all zero: no normal), lrf f64 [B,M,9] (shot_lrf's, or supplied) ->
    (hist i64 [B,M,352], the integer weights in quanta of 2^-32; shot f64 [B,M,352] = hist over its Euclidean norm, zeros
    without a frame or a member; kp_members i32 [B,M])."""
    B, N = _need_frames(pc, count, perm, "shot")
    M = _need_keypoints(pc, keypoints, kp_count, "shot")
    _need_on(normals, "normals", torch.float64, (B, 3, N), pc.device)
    _need_on(lrf, "lrf", torch.float64, (B, M, 9), pc.device)
    if normals is None or lrf is None or not float(radius) > 0.0:
        raise RuntimeError("shot: normals and lrf are required and radius must be positive")
    hist, shot, kp_members = _histogram_rows(B, M, SHOT_WIDTH, pc.device)
    with torch.cuda.device(pc.device), prof.kernel("shot_hist", 40.0 * B * N + (16.0 * SHOT_WIDTH + 88.0) * B * M, keyed=True):
        _lib.check(_lib.lib().usip_shot_hist_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _ptr(normals), _ptr(keypoints),
                                                 _opt_ptr(kp_count), _ptr(lrf), B, N, M, float(radius), _ptr(hist), _ptr(shot),
                                                 _ptr(kp_members), _stream(pc)), "usip_shot_hist_f32")
    return hist, shot, kp_members


# ------------------------------------------------------------------------------------------------ f-21 baseline descriptor: spin images
SPIN_WIDTH = 153
SPIN_STRUCTURES = {"rectangular": 0, "radial": 1}


def spin_image(pc, count, perm, normals, keypoints, kp_count, axes, radius: float, support_angle_cos: float = 0.0,
               structure: str = "rectangular"):
    """f-21: axes f64 [B,M,3] (shot_lrf's z rows, or supplied; a row that is not finite or all zero: no axis), normals f64
    [B,3,N] or None (required only with support_angle_cos > 0) -> (hist i64 [B,M,153], the integer bilinear weights in quanta
    of 2^-40 per member; spin f64 [B,M,153] = hist / (kp_members * 2^40), zeros without an axis or a member; kp_members i32
    [B,M])."""
    B, N = _need_frames(pc, count, perm, "spin")
    M = _need_keypoints(pc, keypoints, kp_count, "spin")
    _need_on(normals, "normals", torch.float64, (B, 3, N), pc.device)
    _need_on(axes, "axes", torch.float64, (B, M, 3), pc.device)
    s = float(support_angle_cos)
    if axes is None or not float(radius) > 0.0 or not 0.0 <= s <= 1.0 or (s > 0.0 and normals is None):
        raise RuntimeError("spin: axes are required, radius must be positive, support_angle_cos in [0, 1], and normals are "
                           "required with a support angle")
    if structure not in SPIN_STRUCTURES:
        raise RuntimeError("spin: structure must be one of %s, got %r" % (sorted(SPIN_STRUCTURES), structure))
    hist, spin, kp_members = _histogram_rows(B, M, SPIN_WIDTH, pc.device)
    with torch.cuda.device(pc.device), prof.kernel("spin_image", (16.0 if s == 0.0 else 40.0) * B * N
                                                   + (16.0 * SPIN_WIDTH + 40.0) * B * M, keyed=True):
        _lib.check(_lib.lib().usip_spin_image_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), _opt_ptr(normals), _ptr(keypoints),
                                                  _opt_ptr(kp_count), _ptr(axes), B, N, M, float(radius), s,
                                                  SPIN_STRUCTURES[structure], _ptr(hist), _ptr(spin), _ptr(kp_members),
                                                  _stream(pc)), "usip_spin_image_f32")
    return hist, spin, kp_members


# ------------------------------------------------------------------------------------------------ f-17 baseline keypoints: SIFT3D
SIFT_NEAREST = 25


def sift_voxel_keys(pc, count, leaf: float):
    """f-17: pc f32 [B,3,N], count i32 [B] or None -> keys i64 [B,N]: the cell of every live point at `leaf` (floor(v / leaf) per
    axis, the grid anchored at the origin), INT64_MAX for a dead slot or a dropped row."""
    B, N = _need_frames(pc, count, tag="sift")
    if not 0.0 < float(leaf) < float("inf"):
        raise RuntimeError("sift: the leaf must be positive and finite")
    keys = torch.empty((B, N), dtype=torch.int64, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("sift_voxel_keys", 20.0 * B * N, keyed=True):
        _lib.check(_lib.lib().usip_sift_voxel_keys_f32(_ptr(pc), _opt_ptr(count), B, N, float(leaf), _ptr(keys), _stream(pc)),
                   "usip_sift_voxel_keys_f32")
    return keys


def sift_voxel_average(pc, field, axis: int, sorted_keys, order):
    """f-17: sorted_keys i64 [B,N] ascending per frame, order i32 [B,N] the input index of each (a stable sort), field f32 [B,N]
    or None (the centroid's coordinate `axis`) -> (cloud f32 [B,3,N], field f32 [B,N], count i32 [B]): one row per distinct
    key, in key order; zeros behind them."""
    B, N = _need_frames(pc, None, tag="sift")
    _need_on(field, "field", torch.float32, (B, N), pc.device)
    _need_on(sorted_keys, "sorted_keys", torch.int64, (B, N), pc.device)
    _need_on(order, "order", torch.int32, (B, N), pc.device)
    if sorted_keys is None or order is None or int(axis) not in (0, 1, 2):
        raise RuntimeError("sift: sorted_keys and order are required and axis must be 0, 1 or 2")
    out = torch.empty((B, 3, N), dtype=torch.float32, device=pc.device)
    out_field = torch.empty((B, N), dtype=torch.float32, device=pc.device)
    cnt = torch.empty((B,), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("sift_voxel_average", 32.0 * B * N, keyed=True):
        _lib.check(_lib.lib().usip_sift_voxel_average_f32(_ptr(pc), _opt_ptr(field), int(axis), _ptr(sorted_keys), _ptr(order),
                                                          B, N, _ptr(out), _ptr(out_field), _ptr(cnt), _stream(pc)),
                   "usip_sift_voxel_average_f32")
    return out, out_field, cnt


def _sigma2(sigma2):
    """the S host float64 values sigma_s^2, as the library reads them"""
    import numpy as np
    a = np.ascontiguousarray(sigma2, dtype=np.float64)
    if a.ndim != 1 or not 4 <= a.shape[0] <= 11:
        raise RuntimeError("sift: sigma2 must hold S = 4 .. 11 float64 values")
    return a


def sift_dog(pc, field, count, perm, sigma2, want_visits: bool = False):
    """f-17: the octave cloud pc f32 [B,3,N] with field f32 [B,N], perm i32 [B,N] (its live rows ascending along x, stable),
    sigma2 the S host float64 values sigma_s^2 -> dog f64 [B,S-1,N]; with want_visits also the 256-point tiles each workgroup
    walked, i32 [B, ceil(N/256)]."""
    B, N = _need_frames(pc, count, perm, "sift")
    _need_on(field, "field", torch.float32, (B, N), pc.device)
    if field is None:
        raise RuntimeError("sift: field is required")
    a = _sigma2(sigma2)
    S = a.shape[0]
    dog = torch.empty((B, S - 1, N), dtype=torch.float64, device=pc.device)
    visits = _visits(B, N, pc.device, want_visits)
    with torch.cuda.device(pc.device), prof.kernel("sift_dog", 16.0 * B * N + 8.0 * B * (S - 1) * N, keyed=True):
        _lib.check(_lib.lib().usip_sift_dog_f32(_ptr(pc), _ptr(field), _opt_ptr(count), _opt_ptr(perm), B, N, S, a.ctypes.data,
                                                _ptr(dog), _opt_ptr(visits), _stream(pc)), "usip_sift_dog_f32")
    return (dog, visits) if want_visits else dog


def sift_nearest(pc, count, perm):
    """f-17: -> idx i32 [B,N,25]: every row's 25 nearest rows of its frame, itself included, ascending (d2, row)."""
    B, N = _need_frames(pc, count, perm, "sift")
    idx = torch.empty((B, N, SIFT_NEAREST), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device), prof.kernel("sift_nearest", (16.0 + 4.0 * SIFT_NEAREST) * B * N, keyed=True):
        _lib.check(_lib.lib().usip_sift_nearest_f32(_ptr(pc), _opt_ptr(count), _opt_ptr(perm), B, N, _ptr(idx), _stream(pc)),
                   "usip_sift_nearest_f32")
    return idx


def sift_extrema(dog, idx, count, min_contrast: float):
    """f-17: dog f64 [B,S-1,N], idx i32 [B,N,25] -> (mask u8 [B,N], scale_index i32 [B,N])."""
    _need(dog, "dog", torch.float64)
    if dog.dim() != 3 or not 3 <= dog.shape[1] <= 10:
        raise RuntimeError("sift: expected dog f64 [B,S-1,N] with S in 4..11")
    B, S1, N = dog.shape
    _need_on(idx, "idx", torch.int32, (B, N, SIFT_NEAREST), dog.device)
    _need_on(count, "count", torch.int32, (B,), dog.device)
    if idx is None or not float(min_contrast) >= 0.0:
        raise RuntimeError("sift: idx is required and min_contrast must be at least 0")
    mask = torch.empty((B, N), dtype=torch.uint8, device=dog.device)
    scale = torch.empty((B, N), dtype=torch.int32, device=dog.device)
    with torch.cuda.device(dog.device), prof.kernel("sift_extrema", (8.0 * S1 + 4.0) * SIFT_NEAREST * B * N, keyed=True):
        _lib.check(_lib.lib().usip_sift_extrema_f32(_ptr(dog), _ptr(idx), _opt_ptr(count), B, N, S1 + 1, float(min_contrast),
                                                    _ptr(mask), _ptr(scale), _stream(dog)), "usip_sift_extrema_f32")
    return mask, scale


# ------------------------------------------------------------------------------------------------ f-12 fast global registration
FGR_MMAX, FGR_ROWS_MAX = 1024, 3000


def _need_fgr(kp1, kp2, n1, n2):
    _need(kp1, "kp1", torch.float32)
    _need(kp2, "kp2", torch.float32)
    if kp1.dim() != 3 or kp1.shape[1] != 3 or kp2.shape != kp1.shape or kp2.device != kp1.device:
        raise RuntimeError("fgr: expected kp1, kp2 f32 [P,3,M] on one device")
    P, _, M = kp1.shape
    if not (1 <= M <= FGR_MMAX and P <= 65535):
        raise RuntimeError("fgr: M must be in 1..%d and P at most 65535 (got P = %d, M = %d)" % (FGR_MMAX, P, M))
    for t, name in ((n1, "n1"), (n2, "n2")):
        if t is None:
            raise RuntimeError("fgr: %s is required" % name)
        _need_on(t, name, torch.int32, (P,), kp1.device)
    return P, M


def fgr_tuples(kp1, kp2, n1, n2, nn12, nn21, seed: int = 0, pair_ids=None, triples=None, want_triples: int = 0):
    """f-12: kp1, kp2 f32 [P,3,M], n1, n2 i32 [P], nn12, nn21 i32 [P,M] (or [P,M,1]) -> dict(mutual i32 [P,M,2], mutual_count
    i32 [P], norm f64 [P,8], rows i32 [P,3000], row_count, trials_walked i32 [P], triples i32 [P,want_triples,3] or None).
    triples i32 [P,T,3]: explicit draws; otherwise Philox draws of (seed, pair_ids)."""
    P, M = _need_fgr(kp1, kp2, n1, n2)
    dev = kp1.device
    nn12, nn21 = nn12.reshape(P, -1), nn21.reshape(P, -1)
    _need_on(nn12, "nn12", torch.int32, (P, M), dev)
    _need_on(nn21, "nn21", torch.int32, (P, M), dev)
    _need_on(pair_ids, "pair_ids", torch.int64, (P,), dev)
    if triples is not None:
        _need(triples, "triples", torch.int32)
        if triples.dim() != 3 or triples.shape[0] != P or triples.shape[1] < 1 or triples.shape[2] != 3 or triples.device != dev:
            raise RuntimeError("fgr: triples must be i32 [P,T,3] on %s" % dev)
    out = {"mutual": torch.empty((P, M, 2), dtype=torch.int32, device=dev),
           "mutual_count": torch.empty((P,), dtype=torch.int32, device=dev),
           "norm": torch.empty((P, 8), dtype=torch.float64, device=dev),
           "rows": torch.empty((P, FGR_ROWS_MAX), dtype=torch.int32, device=dev),
           "row_count": torch.empty((P,), dtype=torch.int32, device=dev),
           "trials_walked": torch.empty((P,), dtype=torch.int32, device=dev),
           "triples": torch.zeros((P, int(want_triples), 3), dtype=torch.int32, device=dev)
           if want_triples and triples is None else None}
    with torch.cuda.device(dev), prof.kernel("fgr_tuples", 32.0 * P * M + 4.0 * P * FGR_ROWS_MAX):
        if triples is None:
            _lib.check(_lib.lib().usip_fgr_tuples_f32(
                _ptr(kp1), _ptr(kp2), _ptr(n1), _ptr(n2), _ptr(nn12), _ptr(nn21), P, M, int(seed) & 0xFFFFFFFFFFFFFFFF,
                _opt_ptr(pair_ids), _ptr(out["mutual"]), _ptr(out["mutual_count"]), _ptr(out["norm"]), _ptr(out["rows"]),
                _ptr(out["row_count"]), _ptr(out["trials_walked"]), _opt_ptr(out["triples"]), int(want_triples),
                _stream(kp1)), "usip_fgr_tuples_f32")
        else:
            _lib.check(_lib.lib().usip_fgr_tuples_explicit_f32(
                _ptr(kp1), _ptr(kp2), _ptr(n1), _ptr(n2), _ptr(nn12), _ptr(nn21), P, M, _ptr(triples), triples.shape[1],
                _ptr(out["mutual"]), _ptr(out["mutual_count"]), _ptr(out["norm"]), _ptr(out["rows"]), _ptr(out["row_count"]),
                _ptr(out["trials_walked"]), _stream(kp1)), "usip_fgr_tuples_explicit_f32")
    return out


def fgr_optimize(kp1, kp2, mutual, mutual_count, norm, rows, row_count, threshold: float):
    """f-12: the 64 Gauss-Newton steps over the tuple rows and the inliers over the mutual rows -> dict(Rt f64 [P,3,4], valid u8
    [P], inlier_mask u8 [P,M], inliers i32 [P])."""
    P, M = _need_fgr(kp1, kp2, mutual_count, row_count)
    dev = kp1.device
    for t, name, dt, shape in ((mutual, "mutual", torch.int32, (P, M, 2)), (norm, "norm", torch.float64, (P, 8)),
                               (rows, "rows", torch.int32, (P, FGR_ROWS_MAX))):
        if t is None:
            raise RuntimeError("fgr: %s is required" % name)
        _need_on(t, name, dt, shape, dev)
    out = {"Rt": torch.empty((P, 3, 4), dtype=torch.float64, device=dev),
           "valid": torch.empty((P,), dtype=torch.uint8, device=dev),
           "inlier_mask": torch.empty((P, M), dtype=torch.uint8, device=dev),
           "inliers": torch.empty((P,), dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev), prof.kernel("fgr_optimize", 32.0 * P * M + 12.0 * P * FGR_ROWS_MAX,
                                             64.0 * 90.0 * P * FGR_ROWS_MAX):
        _lib.check(_lib.lib().usip_fgr_optimize_f32(
            _ptr(kp1), _ptr(kp2), _ptr(mutual), _ptr(mutual_count), _ptr(norm), _ptr(rows), _ptr(row_count), P, M,
            float(threshold), _ptr(out["Rt"]), _ptr(out["valid"]), _ptr(out["inlier_mask"]), _ptr(out["inliers"]),
            _stream(kp1)), "usip_fgr_optimize_f32")
    return out


# ------------------------------------------------------------------------------------------------ f-13 trimmed ICP refinement
ICP_MAX_ITERATIONS = 64
ICP_METRICS = ("point_to_point", "point_to_plane")
ICP_TOL_C = 2.0 * 2.0 ** 0.5 * math.sin(0.5 * 0.009)     # |R - R'|_F of rotations 0.009 rad apart: pcregrigid's default, chordal


def _need_icp(rows, offsets, perm1, frag1, frag2, Rt, mask, order2):
    P = _need_bank(rows, offsets, frag1, frag2, Rt)
    if frag1 is None or Rt is None:
        raise RuntimeError("icp: frag1 and Rt are required")
    dev = rows.device
    _need_on(perm1, "perm1", torch.int32, (rows.shape[0],), dev)
    if perm1 is None:
        raise RuntimeError("icp: perm1 is required")
    _need_on(mask, "mask", torch.uint8, (P,), dev)
    if order2 is not None:
        _need(order2, "order2", torch.int32)
        if order2.dim() != 2 or order2.shape[0] != P or order2.shape[1] < 1 or order2.device != dev:
            raise RuntimeError("icp: order2 must be i32 [P,Lmax] on %s" % dev)
    if P > 65535:
        raise RuntimeError("icp: at most 65535 pairs per call (got %d)" % P)
    return P


def icp_nearest(rows, offsets, perm1, frag1, frag2, Rt, Lmax: int, mask=None, order2=None, want_visits: bool = False):
    """f-13: for every row of fragment 2 moved by Rt f64 [P,3,4] the nearest row of fragment 1 in a CSR bank (rows f32
    [total,>=3], offsets i64 [F+1], perm1 i32 [total]: every fragment's local rows ascending along x) -> (idx i32 [P,Lmax],
    d2 f64 [P,Lmax]): the lowest row index among equal distances, zeros beyond the fragment and where mask u8 [P] is 0.
    order2 i32 [P,Lmax]: which row of fragment 2 each query slot is (a permutation per pair; it never changes a result).
    want_visits: also u64 [P] (as int64), the (query, row) pairs the walk evaluated."""
    P = _need_icp(rows, offsets, perm1, frag1, frag2, Rt, mask, order2)
    Lmax = int(Lmax) if order2 is None else order2.shape[1]
    if not 1 <= Lmax <= 1 << 24:
        raise RuntimeError("icp: Lmax must be in 1..2^24 (got %d)" % Lmax)
    dev = rows.device
    idx = torch.empty((P, Lmax), dtype=torch.int32, device=dev)
    d2 = torch.empty((P, Lmax), dtype=torch.float64, device=dev)
    visits = torch.empty((P,), dtype=torch.int64, device=dev) if want_visits else None
    with torch.cuda.device(dev), prof.kernel("icp_nearest", 28.0 * P * Lmax):
        _lib.check(_lib.lib().usip_icp_nearest_f32(
            *_bank_args(rows, offsets), _ptr(perm1), _ptr(frag1), _ptr(frag2), _ptr(Rt), _opt_ptr(mask), _opt_ptr(order2), P,
            Lmax, _ptr(idx), _ptr(d2), _opt_ptr(visits), _stream(rows)), "usip_icp_nearest_f32")
    return (idx, d2, visits) if want_visits else (idx, d2)


def icp_workspace_bytes(P: int, Lmax: int) -> int:
    need = int(_lib.lib().usip_icp_workspace_bytes(int(P), int(Lmax)))
    if need < 0:
        raise RuntimeError("usip_amd: usip_icp_workspace_bytes: invalid argument (USIP_EINVAL)")
    return need


def icp_refine(rows, offsets, perm1, frag1, frag2, Rt0, Lmax: int, mask=None, order2=None, inlier_ratio: float = 0.3,
               max_iterations: int = 20, tol_t: float = 0.01, tol_c: float = ICP_TOL_C, align_radius: float = 0.05,
               want_visits: bool = False, workspace=None, want_stage_ms: bool = False, want_cuts: bool = False,
               metric: str = "point_to_point", want_sums: bool = False):
    """f-13: trimmed point-to-point ICP from Rt0 f64 [P,3,4] on the bank of icp_nearest -> dict(Rt f64 [P,3,4], iterations
    i32 [P], converged u8 [P], rmse f64 [P], hits i32 [P], ratio f64 [P,2]; visits i64 [P] with want_visits; cut_d2 f64 and
    cut_i i32 [P,max_iterations+1] with want_cuts: the trim's cut (d2*, i*) of every pass, the final pass last).  tol_c bounds
    the Frobenius norm of the change of R (include/usip_hip.h f-13).  No host synchronisation -- unless want_stage_ms asks for
    the measurement stage_ms (host f64 [4]: nearest, trim, fit, the final pass), which waits for the launches.
    metric "point_to_plane" (f-28): the same loop with the plane fit, on a bank whose rows carry their unit normals in
    columns 3..5 (a narrower bank: ValueError); want_sums then adds fit_sums f64 [P,max_iterations,27], every fit's sums."""
    if metric not in ICP_METRICS:
        raise ValueError("icp: metric must be one of %s (got %r)" % (", ".join(ICP_METRICS), metric))
    plane = metric == "point_to_plane"
    if want_sums and not plane:
        raise ValueError("icp: want_sums is the point_to_plane metric's")
    P = _need_icp(rows, offsets, perm1, frag1, frag2, Rt0, mask, order2)
    if plane and rows.shape[1] < 6:
        raise ValueError("icp: the point_to_plane metric needs a bank with normals, rows f32 [total,>=6] (got row_len %d)"
                         % rows.shape[1])
    Lmax = int(Lmax) if order2 is None else order2.shape[1]
    if not 1 <= Lmax <= 1 << 24:
        raise RuntimeError("icp: Lmax must be in 1..2^24 (got %d)" % Lmax)
    if not (0.0 < float(inlier_ratio) <= 1.0 and 0 <= int(max_iterations) <= ICP_MAX_ITERATIONS and float(tol_t) >= 0.0
            and float(tol_c) >= 0.0 and float(align_radius) > 0.0):
        raise RuntimeError("icp: inlier_ratio in (0, 1], max_iterations in 0..%d, tolerances >= 0 and align_radius > 0 "
                           "(got %r, %r, %r, %r, %r)" % (ICP_MAX_ITERATIONS, inlier_ratio, max_iterations, tol_t, tol_c,
                                                        align_radius))
    dev = rows.device
    need = icp_workspace_bytes(P, Lmax)
    if workspace is None:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError("icp: workspace must be contiguous u8 [>= %d] on %s" % (need, dev))
    out = {"Rt": torch.empty((P, 3, 4), dtype=torch.float64, device=dev),
           "iterations": torch.empty((P,), dtype=torch.int32, device=dev),
           "converged": torch.empty((P,), dtype=torch.uint8, device=dev),
           "rmse": torch.empty((P,), dtype=torch.float64, device=dev),
           "hits": torch.empty((P,), dtype=torch.int32, device=dev),
           "ratio": torch.empty((P, 2), dtype=torch.float64, device=dev)}
    visits = torch.empty((P,), dtype=torch.int64, device=dev) if want_visits else None
    stage_ms = (ctypes.c_double * 4)() if want_stage_ms else None
    cut_d2 = torch.empty((P, int(max_iterations) + 1), dtype=torch.float64, device=dev) if want_cuts else None
    cut_i = torch.empty((P, int(max_iterations) + 1), dtype=torch.int32, device=dev) if want_cuts else None
    fit_sums = torch.empty((P, int(max_iterations), 27), dtype=torch.float64, device=dev) if want_sums else None
    name = "usip_icp_refine_plane_f32" if plane else "usip_icp_refine_f32"
    with torch.cuda.device(dev), prof.kernel("icp_refine", 28.0 * P * Lmax * (int(max_iterations) + 1)):
        _lib.check(getattr(_lib.lib(), name)(
            *_bank_args(rows, offsets), _ptr(perm1), _ptr(frag1), _ptr(frag2), _ptr(Rt0), _opt_ptr(mask), _opt_ptr(order2), P,
            Lmax, float(inlier_ratio), int(max_iterations), float(tol_t), float(tol_c), float(align_radius),
            _ptr(workspace), workspace.numel(), _ptr(out["Rt"]),
            _ptr(out["iterations"]), _ptr(out["converged"]), _ptr(out["rmse"]), _ptr(out["hits"]), _ptr(out["ratio"]),
            _opt_ptr(cut_d2), _opt_ptr(cut_i), _opt_ptr(visits), ctypes.addressof(stage_ms) if want_stage_ms else None,
            *((_opt_ptr(fit_sums),) if plane else ()), _stream(rows)), name)
    if want_sums:
        out["fit_sums"] = fit_sums
    if want_visits:
        out["visits"] = visits
    if want_stage_ms:
        out["stage_ms"] = list(stage_ms)
    if want_cuts:
        out["cut_d2"], out["cut_i"] = cut_d2, cut_i
    return out


# ------------------------------------------------------------------------------------------------ f-14 pose-graph pruning
POSEGRAPH_NMAX, POSEGRAPH_MAX_ITERATIONS = 128, 256


def icp_information(rows, offsets, frag1, frag2, idx, d2, mask=None, radius: float = 0.05):
    """f-14: the dense information matrix of computeInformation 'point' over the rows icp_nearest found within `radius`:
    idx i32 [P,Lmax], d2 f64 [P,Lmax] of icp_nearest on the same bank and pairs -> (info f64 [P,6,6], count i32 [P]); zeros
    where mask u8 [P] is 0, a fragment is empty or no row is within the radius."""
    P = _need_bank(rows, offsets, frag1, frag2, None)
    if frag1 is None or idx is None or d2 is None:
        raise RuntimeError("icp_information: frag1, idx and d2 are required")
    dev = rows.device
    _need(idx, "idx", torch.int32)
    if idx.dim() != 2 or idx.shape[0] != P or not 1 <= idx.shape[1] <= 1 << 24 or idx.device != dev:
        raise RuntimeError("icp_information: idx must be i32 [P,Lmax] on %s" % dev)
    Lmax = idx.shape[1]
    _need_on(d2, "d2", torch.float64, (P, Lmax), dev)
    _need_on(mask, "mask", torch.uint8, (P,), dev)
    if P > 65535 or not float(radius) > 0.0:
        raise RuntimeError("icp_information: at most 65535 pairs per call and a positive radius (got %d, %r)" % (P, radius))
    info = torch.empty((P, 6, 6), dtype=torch.float64, device=dev)
    count = torch.empty((P,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), prof.kernel("icp_information", 12.0 * P * Lmax):
        _lib.check(_lib.lib().usip_icp_information_f32(
            *_bank_args(rows, offsets), _ptr(frag1), _ptr(frag2), _ptr(idx), _ptr(d2), _opt_ptr(mask), P, Lmax, float(radius),
            _ptr(info), _ptr(count), _stream(rows)), "usip_icp_information_f32")
    return info, count


def posegraph_workspace_bytes(S: int, Nmax: int, Emax: int) -> int:
    need = int(_lib.lib().usip_posegraph_workspace_bytes(int(S), int(Nmax), int(Emax)))
    if need < 0:
        raise RuntimeError("usip_amd: usip_posegraph_workspace_bytes: invalid argument (USIP_EINVAL)")
    return need


def posegraph_optimize(n, ecount, edge_i, edge_j, X, info, T0, tau2: float = 0.04, prune: float = 0.25,
                       iterations1: int = 32, iterations2: int = 32, workspace=None):
    """f-14: the robust pose-graph optimisation of S scenes in one launch.  n, ecount i32 [S]; edge_i, edge_j i32 [S,Emax]
    sorted by (i, j); X f64 [S,Emax,3,4]; info f64 [S,Emax,6,6]; T0 f64 [S,Nmax,3,4] -> dict(T, weight1, weight2, energy,
    kept u8 [S,Emax], iterations_done i32 [S,2], last_step f64 [S,2], status i32 [S]: 0 done, 1 pivot, 2 a step that is not
    finite, 3 an angle beyond pi, 4 a graph out of shape).  No host synchronisation."""
    _need(T0, "T0", torch.float64)
    if T0.dim() != 4 or tuple(T0.shape[2:]) != (3, 4):
        raise RuntimeError("posegraph: expected T0 f64 [S,Nmax,3,4]")
    S, Nmax = T0.shape[0], T0.shape[1]
    _need(edge_i, "edge_i", torch.int32)
    if edge_i.dim() != 2 or edge_i.shape[0] != S:
        raise RuntimeError("posegraph: expected edge_i i32 [S,Emax]")
    Emax, dev = edge_i.shape[1], T0.device
    if not (S <= 65535 and 2 <= Nmax <= POSEGRAPH_NMAX and 1 <= Emax <= Nmax * (Nmax - 1) // 2):
        raise RuntimeError("posegraph: S <= 65535, 2 <= Nmax <= %d and 1 <= Emax <= Nmax (Nmax - 1) / 2 (got %d, %d, %d)"
                           % (POSEGRAPH_NMAX, S, Nmax, Emax))
    for t, name, dt, shape in ((n, "n", torch.int32, (S,)), (ecount, "ecount", torch.int32, (S,)),
                               (edge_i, "edge_i", torch.int32, (S, Emax)), (edge_j, "edge_j", torch.int32, (S, Emax)),
                               (X, "X", torch.float64, (S, Emax, 3, 4)), (info, "info", torch.float64, (S, Emax, 6, 6))):
        if t is None:
            raise RuntimeError("posegraph: %s is required" % name)
        _need_on(t, name, dt, shape, dev)
    if not (float(tau2) > 0.0 and math.isfinite(float(tau2)) and 0.0 <= float(prune) <= 1.0
            and 0 <= int(iterations1) <= POSEGRAPH_MAX_ITERATIONS and 0 <= int(iterations2) <= POSEGRAPH_MAX_ITERATIONS):
        raise RuntimeError("posegraph: tau2 > 0, prune in [0, 1] and iterations in 0..%d (got %r, %r, %r, %r)"
                           % (POSEGRAPH_MAX_ITERATIONS, tau2, prune, iterations1, iterations2))
    need = posegraph_workspace_bytes(S, Nmax, Emax)
    if workspace is None:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError("posegraph: workspace must be contiguous u8 [>= %d] on %s" % (need, dev))
    out = {"T": torch.empty((S, Nmax, 3, 4), dtype=torch.float64, device=dev),
           "weight1": torch.empty((S, Emax), dtype=torch.float64, device=dev),
           "weight2": torch.empty((S, Emax), dtype=torch.float64, device=dev),
           "energy": torch.empty((S, Emax), dtype=torch.float64, device=dev),
           "kept": torch.empty((S, Emax), dtype=torch.uint8, device=dev),
           "iterations_done": torch.empty((S, 2), dtype=torch.int32, device=dev),
           "last_step": torch.empty((S, 2), dtype=torch.float64, device=dev),
           "status": torch.empty((S,), dtype=torch.int32, device=dev)}
    M = 6.0 * (Nmax - 1)
    steps = int(iterations1) + int(iterations2)
    with torch.cuda.device(dev), prof.kernel("posegraph_optimize", 8.0 * S * steps * M * M, S * steps * M * M * M / 3.0):
        _lib.check(_lib.lib().usip_posegraph_optimize_f64(
            _ptr(n), _ptr(ecount), _ptr(edge_i), _ptr(edge_j), _ptr(X), _ptr(info), _ptr(T0), S, Nmax, Emax, float(tau2),
            float(prune), int(iterations1), int(iterations2), _ptr(workspace), workspace.numel(), _ptr(out["T"]),
            _ptr(out["weight1"]), _ptr(out["weight2"]), _ptr(out["energy"]), _ptr(out["kept"]), _ptr(out["iterations_done"]),
            _ptr(out["last_step"]), _ptr(out["status"]), _stream(T0)), "usip_posegraph_optimize_f64")
    return out


# ------------------------------------------------------------------------------------------------ f-18 scene ground truth
GT_CAP_MAX = 65536


def gt_reach(rows, offsets, perm1, frag1, frag2, Rt, perm2, far: float = 0.03, near: float = 0.006, seed: int = 0,
             pair_ids=None, mask=None):
    """f-18: getGtInfoLog.m's nearest distances at two radii on the CSR bank of icp_nearest: for every row of fragment 2 moved
    by Rt f64 [P,3,4], whether fragment 1 has a row within `far` (class 1) or `near` (class 2).  perm2 i32 [P,Lmax]: fragment
    2's rows ascending along the moved x.  -> dict(cls u8 [P,Lmax] in fragment 2's local row order, hits i32 [P,2] = rows with
    class >= 1 and with class 2, ratio f64 [P,2] = hits[:,0] over n1 and over n2, key i64 [P,Lmax]: the u64 bit patterns of the
    selection keys (63 random bits of (seed, pair id, row) for a class-2 row, all ones = -1 elsewhere)).  Zeros (key -1)
    where mask u8 [P] is 0 or a fragment is empty.  No host synchronisation."""
    P = _need_icp(rows, offsets, perm1, frag1, frag2, Rt, mask, perm2)
    if perm2 is None:
        raise RuntimeError("gt_reach: perm2 is required")
    Lmax, dev = perm2.shape[1], rows.device
    _need_on(pair_ids, "pair_ids", torch.int64, (P,), dev)
    if not (float(near) > 0.0 and float(far) > float(near)) or not 1 <= Lmax <= 1 << 24:
        raise RuntimeError("gt_reach: far > near > 0 and Lmax in 1..2^24 (got %r, %r, %d)" % (far, near, Lmax))
    out = {"cls": torch.empty((P, Lmax), dtype=torch.uint8, device=dev),
           "hits": torch.empty((P, 2), dtype=torch.int32, device=dev),
           "ratio": torch.empty((P, 2), dtype=torch.float64, device=dev),
           "key": torch.empty((P, Lmax), dtype=torch.int64, device=dev)}
    with torch.cuda.device(dev), prof.kernel("gt_reach", 33.0 * P * Lmax):
        _lib.check(_lib.lib().usip_gt_reach_f32(
            *_bank_args(rows, offsets), _ptr(perm1), _ptr(frag1), _ptr(frag2), _ptr(Rt), _ptr(perm2), _opt_ptr(mask), P, Lmax,
            float(far), float(near), int(seed) & 0xFFFFFFFFFFFFFFFF, _opt_ptr(pair_ids), _ptr(out["cls"]), _ptr(out["hits"]),
            _ptr(out["ratio"]), _ptr(out["key"]), _stream(rows)), "usip_gt_reach_f32")
    return out


def gt_information(rows, offsets, frag2, Rt, order, count, Lmax: int):
    """f-18: getGtInfoLog.m's covMat: order i32 [P,cap] (local rows of fragment 2), count i32 [P] -> info f64 [P,6,6] = the sum
    of G'G, G = [I3 | -[q]x], over the first min(count, cap) rows of `order` at q = R b + t; Lmax as gt_reach's (at least the
    longest fragment).  No host synchronisation."""
    P = _need_bank(rows, offsets, None, frag2, Rt)
    if Rt is None or order is None or count is None:
        raise RuntimeError("gt_information: Rt, order and count are required")
    dev = rows.device
    _need(order, "order", torch.int32)
    if order.dim() != 2 or order.shape[0] != P or not 1 <= order.shape[1] <= GT_CAP_MAX or order.device != dev:
        raise RuntimeError("gt_information: order must be i32 [P,cap] with cap in 1..%d on %s" % (GT_CAP_MAX, dev))
    _need_on(count, "count", torch.int32, (P,), dev)
    if P > 65535 or not 1 <= int(Lmax) <= 1 << 24:
        raise RuntimeError("gt_information: at most 65535 pairs per call and Lmax in 1..2^24 (got %d, %d)" % (P, Lmax))
    cap = order.shape[1]
    info = torch.empty((P, 6, 6), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), prof.kernel("gt_information", 16.0 * P * cap):
        _lib.check(_lib.lib().usip_gt_information_f32(
            *_bank_args(rows, offsets), _ptr(frag2), _ptr(Rt), _ptr(order), _ptr(count), P, int(Lmax), cap, _ptr(info),
            _stream(rows)), "usip_gt_information_f32")
    return info


# ------------------------------------------------------------------------------------------------ f-22 the indoor descriptor's CGF triplet loss
CGF_MAX_M, CGF_MAX_C = 65535, 4096


def _cgf_shapes(anc_kp, pos_kp, host: bool):
    for t, name in ((anc_kp, "anc_keypoints"), (pos_kp, "pos_keypoints")):
        _need_host(t, name, torch.float32) if host else _need(t, name, torch.float32)
    if anc_kp.dim() != 3 or anc_kp.shape[1] != 3 or pos_kp.shape != anc_kp.shape or pos_kp.device != anc_kp.device:
        raise RuntimeError("cgf: expected anc_keypoints and pos_keypoints f32 [B,3,M] on one device")
    B, M = anc_kp.shape[0], anc_kp.shape[2]
    if B < 1 or not 1 <= M <= CGF_MAX_M:
        raise RuntimeError("cgf: B >= 1 and M in 1..%d (got %d, %d)" % (CGF_MAX_M, B, M))
    return B, M


def _need_host(t, name: str, dtype):
    if not isinstance(t, torch.Tensor) or t.is_cuda or not t.is_contiguous() or t.dtype != dtype:
        raise RuntimeError("%s must be a contiguous CPU %s tensor" % (name, dtype))


def _cgf_draws(draws, B: int, M: int, device, host: bool):
    """None (Philox) or the dict u1, u2 f32 [B,M,M], u3 f32 [B,M] -> the three tensors or three Nones"""
    if draws is None:
        return None, None, None
    out = []
    for k, shape in (("u1", (B, M, M)), ("u2", (B, M, M)), ("u3", (B, M))):
        t = draws[k]
        _need_host(t, k, torch.float32) if host else _need(t, k, torch.float32)
        if tuple(t.shape) != shape or t.device != device:
            raise RuntimeError("cgf: draws[%r] must be f32 %s on %s" % (k, shape, device))
        out.append(t)
    return tuple(out)


def _cgf_desc(anc_desc, pos_desc, B: int, M: int, host: bool):
    for t, name in ((anc_desc, "anc_descriptors"), (pos_desc, "pos_descriptors")):
        _need_host(t, name, torch.float32) if host else _need(t, name, torch.float32)
    if anc_desc.dim() != 3 or anc_desc.shape[0] != B or anc_desc.shape[2] != M or pos_desc.shape != anc_desc.shape \
            or pos_desc.device != anc_desc.device or not 1 <= anc_desc.shape[1] <= CGF_MAX_C:
        raise RuntimeError("cgf: expected anc_descriptors and pos_descriptors f32 [B,C,M] with C in 1..%d on one device" % CGF_MAX_C)
    return anc_desc.shape[1]


def _cgf_need(t, name: str, dtype, shape, device):
    _need(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise RuntimeError("cgf: %s must be %s %s on %s" % (name, dtype, tuple(shape), device))


def _cgf_u64(v: int) -> int:
    return int(v) & 0xFFFFFFFFFFFFFFFF


def cgf_select(anc_kp, pos_kp, radius: float, draws=None, seed: int = 0, step=0, elem_base: int = 0):
    """f-22: anc_kp, pos_kp f32 [B,3,M] -> (sel i32 [B,M,3] = (j_pos, j_far, j_out), has u8 [B,M], take_far u8 [B,M]).  draws:
    None (Philox: (seed, step, elem_base + b, i, j)) or the dict u1, u2 f32 [B,M,M], u3 f32 [B,M].  step: an int, or a
    one-element int64 DEVICE tensor the kernel reads when it runs (a captured graph draws anew after the word is incremented)."""
    B, M = _cgf_shapes(anc_kp, pos_kp, False)
    dev = anc_kp.device
    u1, u2, u3 = _cgf_draws(draws, B, M, dev, False)
    step_dev = None
    if isinstance(step, torch.Tensor):
        _need(step, "step", torch.int64)
        if step.numel() != 1 or step.device != dev:
            raise RuntimeError("cgf: a tensor step must hold one int64 on %s" % dev)
        step_dev, step = step, 0
    if not float(radius) > 0.0:
        raise RuntimeError("cgf: the radius must be positive")
    sel = torch.empty((B, M, 3), dtype=torch.int32, device=dev)
    has = torch.empty((B, M), dtype=torch.uint8, device=dev)
    take_far = torch.empty((B, M), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), prof.kernel("cgf_select", 24.0 * B * M + 14.0 * B * M, keyed=True):
        _lib.check(_lib.lib().usip_cgf_select_f32(_ptr(anc_kp), _ptr(pos_kp), B, M, float(radius), _opt_ptr(u1), _opt_ptr(u2),
                                                  _opt_ptr(u3), _cgf_u64(seed), _cgf_u64(step), _opt_ptr(step_dev),
                                                  _cgf_u64(elem_base), _ptr(sel), _ptr(has), _ptr(take_far), _stream(anc_kp)),
                   "usip_cgf_select_f32")
    return sel, has, take_far


def _cgf_picks(sel, has, take_far, B: int, M: int, device, host: bool):
    for t, name, dt, shape in ((sel, "sel", torch.int32, (B, M, 3)), (has, "has", torch.uint8, (B, M)),
                               (take_far, "take_far", torch.uint8, (B, M))):
        if t is None:
            continue
        _need_host(t, name, dt) if host else _need(t, name, dt)
        if tuple(t.shape) != shape or t.device != device:
            raise RuntimeError("cgf: %s must be %s %s on %s" % (name, dt, shape, device))


def cgf_loss(anc_desc, pos_desc, anc_sigma, sel, has, take_far, gamma: float, sigma_max: float):
    """f-22: -> (loss f32 [B,M], active f32 [B], dist f64 [B,M,2], coef f64 [B,M]); dist and coef are what the backward needs."""
    B, M = anc_desc.shape[0], anc_desc.shape[2]
    C = _cgf_desc(anc_desc, pos_desc, B, M, False)
    dev = anc_desc.device
    _cgf_need(anc_sigma, "anc_sigmas", torch.float32, (B, M), dev)
    _cgf_picks(sel, has, take_far, B, M, dev, False)
    loss = torch.empty((B, M), dtype=torch.float32, device=dev)
    active = torch.empty((B,), dtype=torch.float32, device=dev)
    dist = torch.empty((B, M, 2), dtype=torch.float64, device=dev)
    coef = torch.empty((B, M), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), prof.kernel("cgf_loss", 12.0 * B * C * M + 50.0 * B * M, keyed=True):
        _lib.check(_lib.lib().usip_cgf_loss_f32(_ptr(anc_desc), _ptr(pos_desc), _ptr(anc_sigma), _ptr(sel), _ptr(has),
                                                _ptr(take_far), B, M, C, float(gamma), float(sigma_max), _ptr(loss), _ptr(active),
                                                _ptr(dist), _ptr(coef), _stream(anc_desc)), "usip_cgf_loss_f32")
    return loss, active, dist, coef


def cgf_loss_backward(anc_desc, pos_desc, sel, take_far, dist, coef, grad_loss):
    """f-22: grad_loss f32 [B,M] -> (d_anc, d_pos) f32 [B,C,M]"""
    B, M = anc_desc.shape[0], anc_desc.shape[2]
    C = _cgf_desc(anc_desc, pos_desc, B, M, False)
    dev = anc_desc.device
    _cgf_picks(sel, None, take_far, B, M, dev, False)
    _cgf_need(dist, "dist", torch.float64, (B, M, 2), dev)
    _cgf_need(coef, "coef", torch.float64, (B, M), dev)
    _cgf_need(grad_loss, "grad_loss", torch.float32, (B, M), dev)
    d_anc, d_pos = torch.empty_like(anc_desc), torch.empty_like(pos_desc)
    with torch.cuda.device(dev), prof.kernel("cgf_loss_backward", 16.0 * B * C * M + 40.0 * B * M, keyed=True):
        _lib.check(_lib.lib().usip_cgf_loss_backward_f32(_ptr(anc_desc), _ptr(pos_desc), _ptr(sel), _ptr(take_far), _ptr(dist),
                                                         _ptr(coef), _ptr(grad_loss), B, M, C, _ptr(d_anc), _ptr(d_pos),
                                                         _stream(anc_desc)), "usip_cgf_loss_backward_f32")
    return d_anc, d_pos


def cgf_select_cpu(anc_kp, pos_kp, radius: float, draws=None, seed: int = 0, step: int = 0, elem_base: int = 0,
                   num_threads: int = 1):
    """Host twin of cgf_select: HOST tensors."""
    B, M = _cgf_shapes(anc_kp, pos_kp, True)
    u1, u2, u3 = _cgf_draws(draws, B, M, anc_kp.device, True)
    if not float(radius) > 0.0:
        raise RuntimeError("cgf: the radius must be positive")
    sel = torch.zeros((B, M, 3), dtype=torch.int32)
    has, take_far = torch.zeros((B, M), dtype=torch.uint8), torch.zeros((B, M), dtype=torch.uint8)
    _lib.check(_lib.lib().usip_cgf_select_f32_cpu(_ptr(anc_kp), _ptr(pos_kp), B, M, float(radius), _opt_ptr(u1), _opt_ptr(u2),
                                                  _opt_ptr(u3), _cgf_u64(seed), _cgf_u64(step), _cgf_u64(elem_base), _ptr(sel),
                                                  _ptr(has), _ptr(take_far), int(num_threads)), "usip_cgf_select_f32_cpu")
    return sel, has, take_far


def cgf_loss_cpu(anc_desc, pos_desc, anc_sigma, sel, has, take_far, gamma: float, sigma_max: float, num_threads: int = 1):
    """Host twin of cgf_loss: HOST tensors."""
    B, M = anc_desc.shape[0], anc_desc.shape[2]
    C = _cgf_desc(anc_desc, pos_desc, B, M, True)
    _need_host(anc_sigma, "anc_sigmas", torch.float32)
    if tuple(anc_sigma.shape) != (B, M):
        raise RuntimeError("cgf: anc_sigmas must be f32 [B,M]")
    _cgf_picks(sel, has, take_far, B, M, anc_desc.device, True)
    loss, active = torch.zeros((B, M), dtype=torch.float32), torch.zeros((B,), dtype=torch.float32)
    dist, coef = torch.zeros((B, M, 2), dtype=torch.float64), torch.zeros((B, M), dtype=torch.float64)
    _lib.check(_lib.lib().usip_cgf_loss_f32_cpu(_ptr(anc_desc), _ptr(pos_desc), _ptr(anc_sigma), _ptr(sel), _ptr(has),
                                                _ptr(take_far), B, M, C, float(gamma), float(sigma_max), _ptr(loss), _ptr(active),
                                                _ptr(dist), _ptr(coef), int(num_threads)), "usip_cgf_loss_f32_cpu")
    return loss, active, dist, coef


def cgf_loss_backward_cpu(anc_desc, pos_desc, sel, take_far, dist, coef, grad_loss, num_threads: int = 1):
    """Host twin of cgf_loss_backward: HOST tensors."""
    B, M = anc_desc.shape[0], anc_desc.shape[2]
    C = _cgf_desc(anc_desc, pos_desc, B, M, True)
    _cgf_picks(sel, None, take_far, B, M, anc_desc.device, True)
    for t, name, dt, shape in ((dist, "dist", torch.float64, (B, M, 2)), (coef, "coef", torch.float64, (B, M)),
                               (grad_loss, "grad_loss", torch.float32, (B, M))):
        _need_host(t, name, dt)
        if tuple(t.shape) != shape:
            raise RuntimeError("cgf: %s must be %s %s" % (name, dt, shape))
    d_anc, d_pos = torch.zeros_like(anc_desc), torch.zeros_like(pos_desc)
    _lib.check(_lib.lib().usip_cgf_loss_backward_f32_cpu(_ptr(anc_desc), _ptr(pos_desc), _ptr(sel), _ptr(take_far), _ptr(dist),
                                                         _ptr(coef), _ptr(grad_loss), B, M, C, _ptr(d_anc), _ptr(d_pos),
                                                         int(num_threads)), "usip_cgf_loss_backward_f32_cpu")
    return d_anc, d_pos


# --------------------------------------------------------------------------- f-25: the indoor head's unit normalisation
def _unit_shapes(x, host: bool, others=()):
    """x f32 [B,C,M] (and same-shaped others) -> (B, C, M)"""
    need = _need_host if host else _need
    need(x, "x", torch.float32)
    if x.dim() != 3:
        raise RuntimeError("unit_columns: expected x f32 [B,C,M]")
    for t, name in others:
        need(t, name, torch.float32)
        if t.shape != x.shape or t.device != x.device:
            raise RuntimeError("unit_columns: %s must be f32 %s on %s" % (name, tuple(x.shape), x.device))
    return tuple(int(v) for v in x.shape)


def _unit_eps(eps) -> float:
    eps = float(eps)
    if not eps >= 0.0:
        raise RuntimeError("unit_columns: eps must be >= 0")
    return eps


def _unit_norm(norm, B: int, M: int, device, host: bool):
    (_need_host if host else _need)(norm, "norm", torch.float32)
    if tuple(norm.shape) != (B, M) or norm.device != device:
        raise RuntimeError("unit_columns: norm must be f32 %s on %s" % ((B, M), device))


def unit_columns(x, eps: float = 1e-5):
    """f-25: x f32 [B,C,M] -> (x / (|x| + eps) f32 [B,C,M], |x| f32 [B,M]), the norm over the channels in float64."""
    B, C, M = _unit_shapes(x, False)
    eps = _unit_eps(eps)
    out = torch.empty_like(x)
    norm = torch.empty((B, M), dtype=torch.float32, device=x.device)
    if x.numel() == 0:                               # no storage to point at: nothing to normalise, the norm of nothing is 0
        return out, norm.zero_()
    with torch.cuda.device(x.device), prof.kernel("unit_columns", 8.0 * B * C * M + 4.0 * B * M, keyed=True):
        _lib.check(_lib.lib().usip_unit_columns_f32(_ptr(x), B, C, M, eps, _ptr(out), _ptr(norm), _stream(x)),
                   "usip_unit_columns_f32")
    return out, norm


def unit_columns_backward(grad, x, norm, eps: float = 1e-5):
    """f-25: grad f32 [B,C,M] (the gradient of unit_columns' first output), x and norm as the forward had them -> dx f32 [B,C,M]"""
    B, C, M = _unit_shapes(x, False, ((grad, "grad"),))
    _unit_norm(norm, B, M, x.device, False)
    eps = _unit_eps(eps)
    dx = torch.empty_like(x)
    if x.numel() == 0:
        return dx
    with torch.cuda.device(x.device), prof.kernel("unit_columns_backward", 12.0 * B * C * M + 4.0 * B * M, keyed=True):
        _lib.check(_lib.lib().usip_unit_columns_backward_f32(_ptr(grad), _ptr(x), _ptr(norm), B, C, M, eps, _ptr(dx), _stream(x)),
                   "usip_unit_columns_backward_f32")
    return dx


def unit_columns_cpu(x, eps: float = 1e-5, num_threads: int = 1):
    """Host twin of unit_columns: HOST tensors."""
    B, C, M = _unit_shapes(x, True)
    eps = _unit_eps(eps)
    out, norm = torch.zeros_like(x), torch.zeros((B, M), dtype=torch.float32)
    if x.numel() == 0:
        return out, norm
    _lib.check(_lib.lib().usip_unit_columns_f32_cpu(_ptr(x), B, C, M, eps, _ptr(out), _ptr(norm), int(num_threads)),
               "usip_unit_columns_f32_cpu")
    return out, norm


def unit_columns_backward_cpu(grad, x, norm, eps: float = 1e-5, num_threads: int = 1):
    """Host twin of unit_columns_backward: HOST tensors."""
    B, C, M = _unit_shapes(x, True, ((grad, "grad"),))
    _unit_norm(norm, B, M, x.device, True)
    eps = _unit_eps(eps)
    dx = torch.zeros_like(x)
    if x.numel() == 0:
        return dx
    _lib.check(_lib.lib().usip_unit_columns_backward_f32_cpu(_ptr(grad), _ptr(x), _ptr(norm), B, C, M, eps, _ptr(dx),
                                                             int(num_threads)), "usip_unit_columns_backward_f32_cpu")
    return dx
