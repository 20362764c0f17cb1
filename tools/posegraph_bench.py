"""Times f-14 on one scene: the nearest pass and the information kernel over the scene's edges, and the robust pose-graph
optimiser per stage and per iteration, with the host twins beside them.

The scene is synthetic: --fragments fragments in a chain with --true-loops true and --false-loops false loop closures (the
generator of tests/posegraph_oracle.py, restated here so that the tool stands alone), and for the information kernel a bank of
--fragments clouds of --points rows each.  Device times are HIP events around the calls, the median of --repeats after a warm
call; the optimiser runs (iterations, 0) and (iterations, iterations) steps, the second stage is their difference.  Prints
ONE JSON line and writes it to --out.

    python tools/posegraph_bench.py [--fragments 57] [--true-loops 200] [--false-loops 30] [--iterations 32] [--points 20000]
                                    [--threads 16] [--repeats 5] [--out profiles/f14_posegraph_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usip_amd import fragments as fr, ops, posegraph as pg            # noqa: E402


def rotvec(v):
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def pose(rot, trans):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotvec(rot), trans
    return T


def make_graph(seed, n, true_loops, false_loops):
    rng = np.random.default_rng(seed)
    poses = [np.eye(4)]
    for _ in range(n - 1):
        poses.append(poses[-1] @ pose(rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.6))
    loops = [(i, j) for i in range(n) for j in range(i + 2, n)]
    rng.shuffle(loops)
    truth = {p: True for p in loops[:true_loops]}
    truth.update({p: False for p in loops[true_loops:true_loops + false_loops]})
    truth.update({(k, k + 1): True for k in range(n - 1)})
    odom, odom_info, loop, loop_info = [], [], [], []
    for i, j in sorted(truth):
        rel = np.linalg.inv(poses[i]) @ poses[j] @ pose(rng.normal(size=3) * 0.003, rng.normal(size=3) * 0.003)
        if not truth[(i, j)]:
            d, t = rng.normal(size=3), rng.normal(size=3)
            rel = rel @ pose(d / np.linalg.norm(d) * 0.8, t / np.linalg.norm(t))
        mat = fr.information_numpy(rng.uniform(-1.5, 1.5, size=(int(rng.integers(200, 2001)), 3)))
        (odom if j - i == 1 else loop).append(fr.LogEntry((i, j, n), rel))
        (odom_info if j - i == 1 else loop_info).append(fr.InfoEntry((i, j, n), mat))
    g = pg.build_graph(odom, odom_info, loop, loop_info)
    want = np.array([truth[(int(i), int(j))] for i, j in zip(g.edge_i, g.edge_j)], np.uint8)
    return g, want


def device_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fragments", type=int, default=57)
    ap.add_argument("--true-loops", type=int, default=200)
    ap.add_argument("--false-loops", type=int, default=30)
    ap.add_argument("--iterations", type=int, default=pg.ITERATIONS)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f14_posegraph_bench.json"))
    args = ap.parse_args()
    dev = torch.device(args.device)
    g, want = make_graph(args.seed, args.fragments, args.true_loops, args.false_loops)
    it = args.iterations

    # the optimiser
    b = {k: torch.from_numpy(v).to(dev) for k, v in pg.pack_graphs([g]).items()}
    ws = torch.empty(ops.posegraph_workspace_bytes(1, g.n, len(g.edge_i)), dtype=torch.uint8, device=dev)
    run = lambda i1, i2: ops.posegraph_optimize(b["n"], b["ecount"], b["edge_i"], b["edge_j"], b["X"], b["info"], b["T0"],
                                                iterations1=i1, iterations2=i2, workspace=ws)
    passes = device_ms(lambda: run(0, 0), args.repeats)
    stage1 = device_ms(lambda: run(it, 0), args.repeats)
    both = device_ms(lambda: run(it, it), args.repeats)
    o = {k: v.cpu().numpy() for k, v in run(it, it).items()}
    twin1 = host_ms(lambda: pg.optimize_cpu([g], iterations1=it, iterations2=0, num_threads=args.threads))
    twin = host_ms(lambda: pg.optimize_cpu([g], iterations1=it, iterations2=it, num_threads=args.threads))
    h, = pg.optimize_cpu([g], iterations1=it, iterations2=it)
    equal = all(np.array_equal(np.asarray(a), np.asarray(c)) for a, c in
                zip(h, pg._unpack([g], o)[0]))

    # the information of every edge: the nearest pass, then the sums
    sc = fr.synthetic_scene(args.seed, args.fragments, args.points, ground_truth=False)
    bank = fr.RefineBank(sc["clouds"], dev)
    near = [(i, i + 1) for i in range(args.fragments - 1)] + [(i, i + 2) for i in range(args.fragments - 2)]
    f1 = torch.tensor([p[0] for p in near], dtype=torch.int32, device=dev)
    f2 = torch.tensor([p[1] for p in near], dtype=torch.int32, device=dev)
    Rt = torch.from_numpy(np.stack([(np.linalg.inv(sc["poses"][i]) @ sc["poses"][j])[:3] for i, j in near])).to(dev).contiguous()
    keys = ops.overlap_keys(bank.rows, bank.offsets, f2, Rt, bank.lmax)
    order2 = torch.argsort(keys, dim=1, stable=True).to(torch.int32)
    nearest = lambda: ops.icp_nearest(bank.rows, bank.offsets, bank.perm, f1, f2, Rt, bank.lmax, None, order2)
    idx, d2 = nearest()
    nearest_ms = device_ms(nearest, args.repeats)
    info_ms = device_ms(lambda: ops.icp_information(bank.rows, bank.offsets, f1, f2, idx, d2, None, pg.INFORMATION_RADIUS),
                        args.repeats)
    _, count = ops.icp_information(bank.rows, bank.offsets, f1, f2, idx, d2, None, pg.INFORMATION_RADIUS)
    hb, k = bank.host(), min(args.host_pairs, len(near))
    hf1, hf2, hRt = f1[:k].cpu().numpy(), f2[:k].cpu().numpy(), Rt[:k].cpu().numpy()
    hidx, hd2 = idx[:k].cpu().numpy(), d2[:k].cpu().numpy()
    twin_nearest = host_ms(lambda: fr.icp_nearest_cpu(hb, hf1, hf2, hRt, None, None, args.threads)) * len(near) / k
    twin_info = host_ms(lambda: pg.icp_information_cpu(hb, hf1, hf2, hidx, hd2, None, pg.INFORMATION_RADIUS, args.threads)) * len(near) / k

    res = {"what": "posegraph_bench", "device": torch.cuda.get_device_name(dev), "fragments": args.fragments,
           "edges": int(len(g.edge_i)), "loops_true": args.true_loops, "loops_false": args.false_loops, "unknowns": 6 * (g.n - 1),
           "iterations": it, "repeats": args.repeats, "threads": args.threads,
           "optimize_ms": {"weight_passes_only": passes, "stage1": stage1 - passes, "stage2": both - stage1,
                           "per_iteration_stage1": (stage1 - passes) / max(it, 1), "per_iteration_stage2": (both - stage1) / max(it, 1),
                           "total": both},
           "optimize_twin_ms": {"stage1": twin1, "total": twin},
           "device_equals_twin": bool(equal), "kept_equals_truth": bool(np.array_equal(o["kept"][0], want)),
           "status": int(o["status"][0]), "last_step": o["last_step"][0].tolist(),
           "information": {"pairs": len(near), "rows_per_fragment_mean": float(np.mean(bank.lengths)),
                           "within_radius_mean": float(count.double().mean()), "nearest_ms": nearest_ms, "information_ms": info_ms,
                           "twin_nearest_ms_scaled": twin_nearest, "twin_information_ms_scaled": twin_info,
                           "twin_pairs_timed": k}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
