"""Loop closures pruned by pose-graph optimisation: the last number of the reference's indoor evaluation,
which is not per pair (evaluation/matlab/eval_indoor: split_txt_compute_G.m -> the robust global optimisation of Choi, Zhou,
Koltun (CVPR 2015) -> loop_evaluation/eval_loop.m, evaluate_optimization.m -> mrEvaluateRegistration.m).

  split_entries            split_txt_compute_G.m: <scene>.log into odometry (j - i == 1) and loop-closure edges, missing
                           odometry edges filled from gt.log / gt.info (or from the pair's own estimate)
  dense_information        computeInformation 'point': one nearest pass on the downsampled fragments, then the sum of A'A over
                           every fragment-1 point a moved fragment-2 point reaches within 0.05 m (csrc/posegraph.hip)
  build_graph              the edges sorted by (i, j), the start poses composed along the odometry chain
  optimize                 the two-stage robust optimisation of a batch of scenes in one launch; include/usip_hip.h (f-14)
                           states the contract, which is this project's own: the reference scores a file made by a tool it
                           does not ship
  refined_entries          the odometry edges and the loop closures that were kept: <scene>_reg_refine_all.log
  evaluate_refined_log     mrEvaluateRegistration: recall and precision of such a log
  prune_pairs / _cpu       the same for the per-pair arrays of fragments.register_pairs, on the device without a host read
  *_cpu                    the same on numpy arrays over the library's host twins (csrc/posegraph_cpu.cpp)
"""
from collections import namedtuple
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, fragments, ops
from .evaluation import _np, _p
from .fragments import InfoEntry, LogEntry, ResultEntry

TAU2, PRUNE, ITERATIONS, INFORMATION_RADIUS = 0.04, 0.25, 32, 0.05       # mrEvaluateRegistration's err2; the 2015 paper's
STATUS = {0: "done", 1: "a pivot that is not finite and positive", 2: "a step that is not finite",
          3: "an angle beyond a half turn", 4: "a graph out of shape"}
Graph = namedtuple("Graph", "n edge_i edge_j X info T0")
GraphResult = namedtuple("GraphResult", "T weight1 weight2 energy kept iterations_done last_step status")
OPTIMIZE_KEYS = ("dense_information", "dense_count", "loop_weight", "loop_kept", "loop_Rt")


# ------------------------------------------------------------------------------------------------ the split
def split_entries(entries: Sequence, infos: Sequence, num_fragments: int, gt: Optional[Sequence] = None,
                  gt_info: Optional[Sequence] = None, fill: Optional[str] = "gt", estimates: Optional[Dict] = None):
    """split_txt_compute_G.m: entries (rows with .info = (i, j, n) and .trans, a result log's) and infos (InfoEntry rows in
    the same order, the dense information of every entry) -> (odom, odom_info, loop, loop_info), LogEntry and InfoEntry rows
    in the order of `entries`.  fill "gt" appends, in gt's order, every (k, k + 1) of gt.log that the odometry list lacks,
    with gt.info's matrix, as the reference does; fill "estimate" appends, in ascending k, every missing (k, k + 1) from
    estimates[(k, k + 1)] = (4 x 4, 6 x 6), the pair's ungated estimate and its dense information -- what a user without
    ground truth has.  After the fill a chain 0 .. num_fragments - 1 that is still incomplete is a ValueError that names the
    pair."""
    if len(entries) != len(infos):
        raise ValueError("split_entries: %d entries but %d information matrices" % (len(entries), len(infos)))
    if fill not in ("gt", "estimate", None):
        raise ValueError("fill must be 'gt', 'estimate' or None (got %r)" % (fill,))
    n = int(num_fragments)
    odom, odom_info, loop, loop_info = [], [], [], []
    for e, m in zip(entries, infos):
        info = tuple(int(v) for v in e.info)
        log, mat = LogEntry(info, np.asarray(e.trans, np.float64).reshape(4, 4)), InfoEntry(info, np.asarray(m.mat, np.float64))
        if info[1] - info[0] == 1:
            odom.append(log)
            odom_info.append(mat)
        else:
            loop.append(log)
            loop_info.append(mat)
    have = {(e.info[0], e.info[1]) for e in odom}
    if fill == "gt":
        if gt is None or gt_info is None:
            raise ValueError("split_entries: fill 'gt' needs gt and gt_info")
        for g, gi in zip(gt, gt_info):
            key = (int(g.info[0]), int(g.info[1]))
            if key[1] - key[0] == 1 and key not in have:
                odom.append(LogEntry(tuple(int(v) for v in g.info), np.asarray(g.trans, np.float64).reshape(4, 4)))
                odom_info.append(InfoEntry(tuple(int(v) for v in gi.info), np.asarray(gi.mat, np.float64)))
                have.add(key)
    elif fill == "estimate":
        for k in range(n - 1):
            if (k, k + 1) not in have and estimates is not None and (k, k + 1) in estimates:
                trans, mat = estimates[(k, k + 1)]
                odom.append(LogEntry((k, k + 1, n), np.asarray(trans, np.float64).reshape(4, 4)))
                odom_info.append(InfoEntry((k, k + 1, n), np.asarray(mat, np.float64).reshape(6, 6)))
                have.add((k, k + 1))
    for k in range(n - 1):
        if (k, k + 1) not in have:
            raise ValueError("split_entries: the odometry chain lacks the pair (%d, %d)" % (k, k + 1))
    return odom, odom_info, loop, loop_info


# ------------------------------------------------------------------------------------------------ dense information
def dense_information(bank, frag1, frag2, Rt, mask=None, radius: float = INFORMATION_RADIUS):
    """computeInformation 'point' for a batch of pairs on the device: bank = fragments.RefineBank (the fragments on the 0.04 m
    grid), frag1, frag2 i32 [P], Rt f64 [P,3,4] the pose the matrix is taken under (the script: pcregrigid's result), mask bool
    or u8 [P] -> (info f64 [P,6,6], count i32 [P]); zeros where mask is 0.  One nearest pass, then the sums.  No host
    synchronisation."""
    Rt = Rt.contiguous()
    m = None if mask is None else mask.to(torch.uint8).contiguous()
    idx, d2 = ops.icp_nearest(bank.rows, bank.offsets, bank.perm, frag1, frag2, Rt, bank.lmax, m,
                              fragments.moved_x_order(bank, frag2, Rt))
    return ops.icp_information(bank.rows, bank.offsets, frag1, frag2, idx, d2, m, radius)


def icp_information_cpu(bank, frag1, frag2, idx, d2, mask=None, radius: float = INFORMATION_RADIUS, num_threads: int = 1):
    """ops.icp_information on numpy arrays over the host twin."""
    args, alive = fragments._host_bank_args(bank)
    f2 = _np(frag2, np.int32, "frag2")
    P = f2.shape[0]
    f1 = _np(frag1, np.int32, "frag1", (P,))
    ix = _np(idx, np.int32, "idx")
    if ix.ndim != 2 or ix.shape[0] != P or not 1 <= ix.shape[1] <= 1 << 24:
        raise RuntimeError("icp_information: idx must be i32 [P,Lmax]")
    dd = _np(d2, np.float64, "d2", ix.shape)
    if P > 65535 or not float(radius) > 0.0:
        raise RuntimeError("icp_information: at most 65535 pairs per call and a positive radius (got %d, %r)" % (P, radius))
    m = None if mask is None else _np(np.asarray(mask).astype(np.uint8), np.uint8, "mask", (P,))
    info, count = np.zeros((P, 6, 6)), np.zeros(P, np.int32)
    _lib.check(_lib.lib().usip_icp_information_f32_cpu(
        *args, _p(f1), _p(f2), _p(ix), _p(dd), _p(m), P, ix.shape[1], float(radius), _p(info), _p(count), int(num_threads)),
        "usip_icp_information_f32_cpu")
    return info, count


def dense_information_cpu(bank, frag1, frag2, Rt, mask=None, radius: float = INFORMATION_RADIUS, num_threads: int = 1):
    """dense_information on numpy arrays over the host twins; bank = fragments.HostBank of the downsampled fragments."""
    idx, d2 = fragments.icp_nearest_cpu(bank, frag1, frag2, Rt, mask, None, num_threads)
    return icp_information_cpu(bank, frag1, frag2, idx, d2, mask, radius, num_threads)


# ------------------------------------------------------------------------------------------------ the graph
def _compose(A, B):
    """A B of [.., 3, 4] rigid transforms, elementwise and every sum from the left: numpy and torch give the same bits."""
    cols = []
    for c in range(4):
        v = (A[..., :, 0] * B[..., 0, c][..., None] + A[..., :, 1] * B[..., 1, c][..., None]) \
            + A[..., :, 2] * B[..., 2, c][..., None]
        cols.append(v + A[..., :, 3] if c == 3 else v)
    return (torch.stack if isinstance(A, torch.Tensor) else np.stack)(cols, -1)


def _inverse(A):
    """[R' | -(R' t)] of [.., 3, 4]"""
    R = A[..., :, :3]
    Rt = R.transpose(-1, -2) if isinstance(A, torch.Tensor) else np.swapaxes(R, -1, -2)
    t = A[..., :, 3]
    v = -((Rt[..., :, 0] * t[..., 0][..., None] + Rt[..., :, 1] * t[..., 1][..., None]) + Rt[..., :, 2] * t[..., 2][..., None])
    return (torch.cat if isinstance(A, torch.Tensor) else np.concatenate)((Rt, v[..., None]), -1)


def chain_poses(X_chain):
    """T_0 = I, T_(k+1) = T_k X_(k,k+1) from X_chain [n - 1, 3, 4] -> [n, 3, 4] (numpy or torch, the same bits)."""
    lib_t = isinstance(X_chain, torch.Tensor)
    eye = torch.eye(3, 4, dtype=torch.float64, device=X_chain.device) if lib_t else np.eye(3, 4)
    out = [eye]
    for k in range(X_chain.shape[0]):
        out.append(_compose(out[-1], X_chain[k]))
    return (torch.stack if lib_t else np.stack)(out)


def build_graph(odom: Sequence, odom_info: Sequence, loop: Sequence, loop_info: Sequence,
                num_fragments: Optional[int] = None) -> Graph:
    """The four lists of split_entries -> Graph(n, edge_i, edge_j i32 [E], X f64 [E,3,4], info f64 [E,6,6], T0 f64 [n,3,4]):
    the edges sorted by (i, j) whatever order they came in, the start poses composed along the odometry chain.  ValueError:
    an edge with i >= j or a fragment outside 0 .. n - 1, a pair given twice, a chain that lacks a pair."""
    rows = list(zip(list(odom) + list(loop), list(odom_info) + list(loop_info)))
    if not rows:
        raise ValueError("build_graph: no edges")
    n = int(num_fragments if num_fragments is not None else rows[0][0].info[2])
    if not 2 <= n <= ops.POSEGRAPH_NMAX:
        raise ValueError("build_graph: 2 .. %d fragments (got %d)" % (ops.POSEGRAPH_NMAX, n))
    seen = {}
    for e, m in rows:
        i, j = int(e.info[0]), int(e.info[1])
        if (int(m.info[0]), int(m.info[1])) != (i, j):
            raise ValueError("build_graph: the information of (%d, %d) is listed at the edge (%d, %d)" % (m.info[0], m.info[1], i, j))
        if not 0 <= i < j < n:
            raise ValueError("build_graph: the edge (%d, %d) needs 0 <= i < j < %d" % (i, j, n))
        if (i, j) in seen:
            raise ValueError("build_graph: the pair (%d, %d) is given twice" % (i, j))
        seen[(i, j)] = (np.asarray(e.trans, np.float64).reshape(4, 4)[:3], np.asarray(m.mat, np.float64).reshape(6, 6))
    for k in range(n - 1):
        if (k, k + 1) not in seen:
            raise ValueError("build_graph: the odometry chain lacks the pair (%d, %d)" % (k, k + 1))
    keys = sorted(seen)
    X = np.ascontiguousarray(np.stack([seen[k][0] for k in keys]))
    info = np.ascontiguousarray(np.stack([seen[k][1] for k in keys]))
    T0 = chain_poses(np.stack([seen[(k, k + 1)][0] for k in range(n - 1)]))
    return Graph(n, np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32), X, info,
                 np.ascontiguousarray(T0))


def pack_graphs(graphs: Sequence[Graph]) -> Dict[str, np.ndarray]:
    """A batch of graphs, padded to one shape: what the library's entry points take."""
    if not graphs:
        raise ValueError("pack_graphs: no graphs")
    S, Nmax, Emax = len(graphs), max(g.n for g in graphs), max(max(len(g.edge_i) for g in graphs), 1)
    Nmax = max(Nmax, 2)
    b = {"n": np.array([g.n for g in graphs], np.int32), "ecount": np.array([len(g.edge_i) for g in graphs], np.int32),
         "edge_i": np.zeros((S, Emax), np.int32), "edge_j": np.zeros((S, Emax), np.int32), "X": np.zeros((S, Emax, 3, 4)),
         "info": np.zeros((S, Emax, 6, 6)), "T0": np.zeros((S, Nmax, 3, 4))}
    for s, g in enumerate(graphs):
        E = len(g.edge_i)
        b["edge_i"][s, :E], b["edge_j"][s, :E] = g.edge_i, g.edge_j
        b["X"][s, :E], b["info"][s, :E] = np.asarray(g.X, np.float64).reshape(E, 3, 4), np.asarray(g.info, np.float64).reshape(E, 6, 6)
        b["T0"][s, :g.n] = np.asarray(g.T0, np.float64).reshape(-1, 3, 4)[:g.n]
    return b


def _check_scalars(tau2, prune, iterations1, iterations2):
    lim = ops.POSEGRAPH_MAX_ITERATIONS
    if not (float(tau2) > 0.0 and np.isfinite(float(tau2)) and 0.0 <= float(prune) <= 1.0 and 0 <= int(iterations1) <= lim
            and 0 <= int(iterations2) <= lim):
        raise RuntimeError("posegraph: tau2 > 0, prune in [0, 1] and iterations in 0..%d (got %r, %r, %r, %r)"
                           % (lim, tau2, prune, iterations1, iterations2))


def optimize_arrays_cpu(b: Dict[str, np.ndarray], tau2: float = TAU2, prune: float = PRUNE, iterations1: int = ITERATIONS,
                        iterations2: int = ITERATIONS, num_threads: int = 1) -> Dict[str, np.ndarray]:
    """usip_posegraph_optimize_f64_cpu on the arrays of pack_graphs -> the arrays of ops.posegraph_optimize."""
    T0 = _np(b["T0"], np.float64, "T0")
    if T0.ndim != 4 or T0.shape[2:] != (3, 4):
        raise ValueError("expected T0 f64 [S,Nmax,3,4]")
    S, Nmax = T0.shape[:2]
    ei = _np(b["edge_i"], np.int32, "edge_i")
    if ei.ndim != 2 or ei.shape[0] != S:
        raise ValueError("expected edge_i i32 [S,Emax]")
    Emax = ei.shape[1]
    ej, n, ec = _np(b["edge_j"], np.int32, "edge_j", (S, Emax)), _np(b["n"], np.int32, "n", (S,)), _np(b["ecount"], np.int32, "ecount", (S,))
    X, info = _np(b["X"], np.float64, "X", (S, Emax, 3, 4)), _np(b["info"], np.float64, "info", (S, Emax, 6, 6))
    out = {"T": np.zeros((S, Nmax, 3, 4)), "weight1": np.zeros((S, Emax)), "weight2": np.zeros((S, Emax)),
           "energy": np.zeros((S, Emax)), "kept": np.zeros((S, Emax), np.uint8), "iterations_done": np.zeros((S, 2), np.int32),
           "last_step": np.zeros((S, 2)), "status": np.zeros(S, np.int32)}
    _lib.check(_lib.lib().usip_posegraph_optimize_f64_cpu(
        _p(n), _p(ec), _p(ei), _p(ej), _p(X), _p(info), _p(T0), S, Nmax, Emax, float(tau2), float(prune), int(iterations1),
        int(iterations2), _p(out["T"]), _p(out["weight1"]), _p(out["weight2"]), _p(out["energy"]), _p(out["kept"]),
        _p(out["iterations_done"]), _p(out["last_step"]), _p(out["status"]), int(num_threads)),
        "usip_posegraph_optimize_f64_cpu")
    return out


def _unpack(graphs, o) -> List[GraphResult]:
    out = []
    for s, g in enumerate(graphs):
        E = len(g.edge_i)
        out.append(GraphResult(o["T"][s, :g.n], o["weight1"][s, :E], o["weight2"][s, :E], o["energy"][s, :E], o["kept"][s, :E],
                               o["iterations_done"][s], o["last_step"][s], int(o["status"][s])))
    return out


def optimize_cpu(graphs: Sequence[Graph], tau2: float = TAU2, prune: float = PRUNE, iterations1: int = ITERATIONS,
                 iterations2: int = ITERATIONS, num_threads: int = 1) -> List[GraphResult]:
    """optimize over the host twin."""
    _check_scalars(tau2, prune, iterations1, iterations2)
    return _unpack(graphs, optimize_arrays_cpu(pack_graphs(graphs), tau2, prune, iterations1, iterations2, num_threads))


def optimize(graphs: Sequence[Graph], tau2: float = TAU2, prune: float = PRUNE, iterations1: int = ITERATIONS,
             iterations2: int = ITERATIONS, device="cuda") -> List[GraphResult]:
    """The two-stage robust optimisation of every graph, all scenes in one launch -> GraphResult rows on the host: T f64
    [n,3,4] (fragment k into fragment 0's frame), weight1 (the line process after stage 1: a loop closure below `prune` is
    dropped), weight2 and energy after stage 2, kept u8 [E], iterations_done i32 [2], last_step f64 [2], status (STATUS)."""
    _check_scalars(tau2, prune, iterations1, iterations2)
    dev = torch.device(device)
    b = {k: torch.from_numpy(v).to(dev) for k, v in pack_graphs(graphs).items()}
    o = ops.posegraph_optimize(b["n"], b["ecount"], b["edge_i"], b["edge_j"], b["X"], b["info"], b["T0"], tau2, prune,
                               iterations1, iterations2)
    return _unpack(graphs, {k: v.cpu().numpy() for k, v in o.items()})


def refined_entries(graph: Graph, result: GraphResult, transform: str = "edge") -> List[LogEntry]:
    """One LogEntry per odometry edge and per loop closure that was kept, in the graph's order: what
    <scene>_reg_refine_all.log holds.  transform "edge" keeps the edge's own transform, "graph" writes T_i^-1 T_j of the
    optimised poses."""
    if transform not in ("edge", "graph"):
        raise ValueError("transform must be 'edge' or 'graph' (got %r)" % (transform,))
    out = []
    for e in range(len(graph.edge_i)):
        i, j = int(graph.edge_i[e]), int(graph.edge_j[e])
        if j - i == 1 or result.kept[e]:
            Rt = graph.X[e] if transform == "edge" else _compose(_inverse(result.T[i]), result.T[j])
            out.append(LogEntry((i, j, graph.n), fragments.to4x4(Rt)))
    return out


def evaluate_refined_log(entries: Sequence, gt: Sequence, gt_info: Sequence, err2: float = TAU2) -> Dict:
    """mrEvaluateRegistration: fragments.evaluate_log on LogEntry rows, without the inlier statistics."""
    rows = [ResultEntry(tuple(e.info), e.trans, 0, 0.0, None) for e in entries]
    out = fragments.evaluate_log(rows, gt, gt_info, err2)
    return {k: v for k, v in out.items() if not k.startswith("inlier_")}


# ------------------------------------------------------------------------------------------------ files
def write_split(directory, scene: str, odom, odom_info, loop, loop_info):
    """<scene>_odom.log/.info and <scene>_loop.log/.info, in mrWriteLog's and mrWriteInfo's formats -> the four paths."""
    paths = [os.path.join(str(directory), scene + suffix) for suffix in ("_odom.log", "_odom.info", "_loop.log", "_loop.info")]
    fragments.write_log(paths[0], odom)
    fragments.write_info(paths[1], odom_info)
    fragments.write_log(paths[2], loop)
    fragments.write_info(paths[3], loop_info)
    return paths


def read_split(directory, scene: str):
    d = str(directory)
    return (fragments.read_log(os.path.join(d, scene + "_odom.log")), fragments.read_info(os.path.join(d, scene + "_odom.info")),
            fragments.read_log(os.path.join(d, scene + "_loop.log")), fragments.read_info(os.path.join(d, scene + "_loop.info")))


def write_refined(directory, scene: str, entries: Sequence) -> str:
    path = os.path.join(str(directory), scene + "_reg_refine_all.log")
    fragments.write_log(path, entries)
    return path


# ------------------------------------------------------------------------------------------------ per-pair arrays
class EdgePlan:
    """What the host knows about a scene's candidate edges before anything is read from the device: the pairs that were
    run, sorted by (i, j), plus, under fill "gt", the odometry pairs of gt.log (they stand in where the pair did not pass the
    gate, or was not run).  src[c] is the candidate's index among the pairs, or -1."""

    def __init__(self, pair_ij: Sequence, num_fragments: int, fill: Optional[str] = "gt", gt=None, gt_info=None):
        if fill not in ("gt", "estimate", None):
            raise ValueError("fill must be 'gt', 'estimate' or None (got %r)" % (fill,))
        self.n, self.fill = int(num_fragments), fill
        if not 2 <= self.n <= ops.POSEGRAPH_NMAX:
            raise ValueError("optimize: 2 .. %d fragments (got %d)" % (ops.POSEGRAPH_NMAX, self.n))
        cand = {}
        for p, (i, j) in enumerate(pair_ij):
            i, j = int(i), int(j)
            if not 0 <= i < j < self.n:
                raise ValueError("optimize: the pair (%d, %d) needs 0 <= i < j < %d" % (i, j, self.n))
            if (i, j) in cand:
                raise ValueError("optimize: the pair (%d, %d) is given twice" % (i, j))
            cand[(i, j)] = [p, None]
        if fill == "gt":
            if gt is None or gt_info is None:
                raise ValueError("optimize: fill 'gt' needs gt and gt_info")
            for g, gi in zip(gt, gt_info):
                i, j = int(g.info[0]), int(g.info[1])
                if j - i == 1 and 0 <= i and j < self.n:
                    cand.setdefault((i, j), [-1, None])[1] = (np.asarray(g.trans, np.float64).reshape(4, 4)[:3],
                                                             np.asarray(gi.mat, np.float64).reshape(6, 6))
        for k in range(self.n - 1):
            if (k, k + 1) not in cand:
                raise ValueError("optimize: the odometry chain lacks the pair (%d, %d)" % (k, k + 1))
        keys = sorted(cand)
        self.C = len(keys)
        self.ci, self.cj = np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32)
        self.src = np.array([cand[k][0] for k in keys], np.int64)
        self.has_fill = np.array([cand[k][1] is not None for k in keys], bool)
        self.fill_X = np.stack([cand[k][1][0] if cand[k][1] is not None else np.eye(3, 4) for k in keys])
        self.fill_info = np.stack([cand[k][1][1] if cand[k][1] is not None else np.zeros((6, 6)) for k in keys])
        self.odometry = self.cj - self.ci == 1
        self.estimate = self.odometry & (self.src >= 0) if fill == "estimate" else np.zeros(self.C, bool)
        where = {k: c for c, k in enumerate(keys)}
        self.chain = np.array([where[(k, k + 1)] for k in range(self.n - 1)], np.int64)
        self.of_pair = np.full(len(pair_ij), 0, np.int64)
        self.of_pair[self.src[self.src >= 0]] = np.nonzero(self.src >= 0)[0]

    def check_chain(self, gate):
        """After the host has the gate: with fill None a chain pair that did not pass is an error that names it."""
        g = np.asarray(gate).astype(bool)
        for k, c in enumerate(self.chain):
            ok = (self.src[c] >= 0 and g[self.src[c]]) or self.has_fill[c] or self.estimate[c]
            if not ok:
                raise ValueError("optimize: the odometry chain lacks the pair (%d, %d)" % (k, k + 1))


def _prune(plan: EdgePlan, gate, X, info, args, run, lib_t, dev=None):
    """The shared body of prune_pairs and prune_pairs_cpu: nothing here depends on a value of gate, X or info."""
    C, n = plan.C, plan.n
    if lib_t:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        where, cumsum = torch.where, lambda a: torch.cumsum(a, 0)
        zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
    else:
        up = lambda a: np.ascontiguousarray(a)
        where, cumsum = np.where, lambda a: np.cumsum(a, 0)
        zeros = lambda shape, dt: np.zeros(shape, dt)
        i32, i64, f64, u8 = np.int32, np.int64, np.float64, np.uint8
    src = up(np.maximum(plan.src, 0))
    ran, has_fill, est = up(plan.src >= 0), up(plan.has_fill), up(plan.estimate)
    g = (gate != 0)[src] & ran
    include = g | has_fill | est
    own = (g | est)[:, None, None]
    Xc = where(own, X[src], up(plan.fill_X))
    Lc = where(own, info[src], up(plan.fill_info))
    inc = include.to(i64) if lib_t else include.astype(i64)
    pos = cumsum(inc) - 1
    slot = where(include, pos, pos * 0 + C)                        # a candidate left out lands in a slot that is cut off
    def scatter(vals, shape, dt):
        buf = zeros((C + 1,) + shape, dt)
        buf[slot] = vals
        return buf[:C]
    b = {"n": up(np.array([n], np.int32)), "ecount": (inc.sum().reshape(1)).to(i32) if lib_t else inc.sum().reshape(1).astype(i32),
         "edge_i": scatter(up(plan.ci), (), i32)[None], "edge_j": scatter(up(plan.cj), (), i32)[None],
         "X": scatter(Xc, (3, 4), f64)[None], "info": scatter(Lc, (6, 6), f64)[None],
         "T0": chain_poses(Xc[up(plan.chain)])[None]}
    b = {k: (v.contiguous() if lib_t else np.ascontiguousarray(v)) for k, v in b.items()}
    o = run(b, **args)
    at = where(include, pos, pos * 0)
    w1 = where(include, o["weight1"][0][at], o["weight1"][0][at] * 0)
    kept = where(include, o["kept"][0][at], o["kept"][0][at] * 0)
    T = o["T"][0]
    rel = _compose(_inverse(T[up(plan.ci.astype(np.int64))]), T[up(plan.cj.astype(np.int64))])
    of_pair = up(plan.of_pair)
    return {"loop_weight": w1[of_pair], "loop_kept": kept[of_pair], "loop_Rt": rel[of_pair], "loop_status": o["status"],
            "loop_iterations": o["iterations_done"][0]}


def split_optimize_args(args: Optional[Dict]):
    """optimize_args -> (the optimiser's scalars, fill or the string "default", transform, radius); an unknown key is a
    ValueError."""
    a = {"tau2": TAU2, "prune": PRUNE, "iterations1": ITERATIONS, "iterations2": ITERATIONS}
    args = dict(args or {})
    extra = set(args) - set(a) - {"fill", "transform", "radius"}
    if extra:
        raise ValueError("optimize_args: unknown keys %s" % sorted(extra))
    a.update({k: v for k, v in args.items() if k in a})
    _check_scalars(a["tau2"], a["prune"], a["iterations1"], a["iterations2"])
    fill, transform = args.get("fill", "default"), args.get("transform", "edge")
    if fill not in ("gt", "estimate", None, "default") or transform not in ("edge", "graph"):
        raise ValueError("optimize_args: fill is 'gt', 'estimate' or None and transform 'edge' or 'graph' (got %r, %r)"
                         % (fill, transform))
    return a, fill, transform, float(args.get("radius", INFORMATION_RADIUS))


def _optimize_args(args):
    return split_optimize_args(args)[0]


def plan_for(pairs: Sequence, fragment_ids: Sequence[int], gt, gt_info, optimize_args: Optional[Dict]) -> EdgePlan:
    """The EdgePlan of a scene whose pairs (a, b) are fragment ids; the fragments number as gt.log says, else one more than
    the largest id.  fill defaults to "gt" with a ground truth and to "estimate" without."""
    _, fill, _, _ = split_optimize_args(optimize_args)
    if fill == "default":
        fill = "gt" if gt is not None and gt_info is not None else "estimate"
    n = int(gt[0].info[2]) if gt else int(max(fragment_ids)) + 1
    return EdgePlan([(int(a), int(b)) for a, b in pairs], n, fill, gt, gt_info)


def summarize_loops(per_pair: Dict[str, np.ndarray], fragment_ids: Sequence[int], gt, gt_info, gate: str, transform: str,
                    optimize_args: Optional[Dict], num_threads: int = 1) -> Dict:
    """What fragments.summarize adds under optimize_args, on the host: the pairs under `gate` as a pose graph with the
    transforms per_pair[transform] and the matrices per_pair["dense_information"]; pruned by the host twin unless per_pair
    already holds loop_kept (FragmentEvaluator ran it on the device).  -> loops_in (loop closures that entered), loops_kept,
    refined_entries (LogEntry rows of <scene>_reg_refine_all.log), split (odom, odom_info, loop, loop_info: the four
    lists of split_txt_compute_G.m), and with a ground truth loop_recall and loop_precision (mrEvaluateRegistration)."""
    if "dense_information" not in per_pair:
        raise ValueError("optimize needs the per-pair dense_information (register_pairs with dense_radius)")
    _, _, how, _ = split_optimize_args(optimize_args)
    pairs = [(int(fragment_ids[a]), int(fragment_ids[b])) for a, b in zip(per_pair["frag1"], per_pair["frag2"])]
    plan = plan_for(pairs, fragment_ids, gt, gt_info, optimize_args)
    g = np.asarray(per_pair[gate]).astype(bool)
    plan.check_chain(g)
    if "loop_kept" not in per_pair:
        per_pair.update(prune_pairs_cpu(plan, g, per_pair[transform], per_pair["dense_information"], optimize_args, num_threads))
    odom, odom_info, loop, loop_info, refined = [], [], [], [], []
    loops_in = loops_kept = 0
    for c in range(plan.C):
        i, j, p = int(plan.ci[c]), int(plan.cj[c]), int(plan.src[c])
        own = p >= 0 and (g[p] or plan.estimate[c])
        if not (own or plan.has_fill[c]):
            continue
        tag = (i, j, plan.n)
        X = fragments.to4x4(per_pair[transform][p] if own else plan.fill_X[c])
        L = per_pair["dense_information"][p] if own else plan.fill_info[c]
        (odom if j - i == 1 else loop).append(LogEntry(tag, X))
        (odom_info if j - i == 1 else loop_info).append(InfoEntry(tag, np.asarray(L, np.float64)))
        kept = j - i == 1 or bool(per_pair["loop_kept"][p])
        loops_in += j - i > 1
        loops_kept += j - i > 1 and kept
        if kept:
            refined.append(LogEntry(tag, fragments.to4x4(per_pair["loop_Rt"][p]) if how == "graph" and p >= 0 else X))
    out = {"loops_in": int(loops_in), "loops_kept": int(loops_kept), "refined_entries": refined,
           "split": (odom, odom_info, loop, loop_info)}
    if gt is not None and gt_info is not None:
        score = evaluate_refined_log(refined, gt, gt_info)
        out.update(loop_recall=score["recall"], loop_precision=score["precision"])
    return out


def prune_pairs(plan: EdgePlan, gate, X, info, optimize_args: Optional[Dict] = None) -> Dict[str, torch.Tensor]:
    """The scene's graph from per-pair device tensors -- gate bool [P] (the pairs the log would hold), X f64 [P,3,4] (the
    log's transforms), info f64 [P,6,6] (their dense information) -- optimised on the device -> loop_weight f64 [P] (the
    line process after stage 1), loop_kept u8 [P] (the pair is an edge of the refined log), loop_Rt f64 [P,3,4] (T_i^-1 T_j
    of the optimised poses), loop_status i32 [1], loop_iterations i32 [2].  No host synchronisation: the edges are compacted
    by a prefix sum, never listed on the host."""
    run = lambda b, **a: ops.posegraph_optimize(b["n"], b["ecount"], b["edge_i"], b["edge_j"], b["X"], b["info"], b["T0"], **a)
    return _prune(plan, gate, X.contiguous(), info.contiguous(), _optimize_args(optimize_args), run, True, X.device)


def prune_pairs_cpu(plan: EdgePlan, gate, X, info, optimize_args: Optional[Dict] = None, num_threads: int = 1):
    """prune_pairs on numpy arrays over the host twin."""
    run = lambda b, **a: optimize_arrays_cpu(b, num_threads=num_threads, **a)
    return _prune(plan, np.asarray(gate), np.asarray(X, np.float64), np.asarray(info, np.float64),
                  _optimize_args(optimize_args), run, False)
